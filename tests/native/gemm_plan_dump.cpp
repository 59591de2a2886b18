// Host driver of tests/test_gemm_plan.py: one GemmCall per stdin line (the fields in the order read below), one
// GemmPlan per stdout line as "name=value" pairs. Built with the host C++ compiler against gemm_plan.h alone.
#include <cstdio>

#include "gemm_plan.h"

int main() {
  nsdb::GemmCall c;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %d %lld %d", &c.M, &c.N, &c.K, &c.batch,
                    &c.splits, &c.cfg, &c.epi, &c.mfma, &c.fixup, &c.kinter, &c.out_f32, &c.accumulate, &c.bias_mode,
                    &c.lda, &c.ldb, &c.ldc, &c.sC, &c.c_align, &c.seg_k, &c.has_ws) == 20) {
    const nsdb::GemmPlan p = nsdb::gemm_plan(c);
    std::printf("rc=%d cfg=%d tbm=%d tbn=%d tiles_m=%d tiles_n=%d splits=%d kchunk=%d wgs=%lld vec_ws=%d vec_c=%d "
                "direct_epi=%d kernel=%s kinter=%d reducer=%s reduce_blocks=%d prefetch_eligible=%d\n",
                p.rc, p.cfg, p.tbm, p.tbn, p.tiles_m, p.tiles_n, p.splits, p.kchunk, p.wgs, p.vec_ws, p.vec_c,
                p.direct_epi, nsdb::gemm_kernel_name(p.kernel), p.kinter, nsdb::gemm_reducer_name(p.reducer),
                p.reduce_blocks, p.prefetch_eligible);
  }
  return 0;
}
