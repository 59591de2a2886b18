// Host driver of tests/test_gemm_plan_packed.py: one GemmCall per stdin line (the fields of gemm_plan_dump.cpp, then
// `packed`), one stdout line with two GemmPlans as "name=value" pairs: the plan of the call as given, then ("|") the
// plan of the same call without the packed request. Built with the host C++ compiler against gemm_plan.h alone.
#include <cstdio>

#include "gemm_plan.h"

static void show(const nsdb::GemmPlan& p, const char* end) {
  std::printf("rc=%d cfg=%d tbm=%d tbn=%d tiles_m=%d tiles_n=%d splits=%d kchunk=%d wgs=%lld vec_ws=%d vec_c=%d "
              "direct_epi=%d kernel=%s kinter=%d reducer=%s reduce_blocks=%d prefetch_eligible=%d packed=%d%s",
              p.rc, p.cfg, p.tbm, p.tbn, p.tiles_m, p.tiles_n, p.splits, p.kchunk, p.wgs, p.vec_ws, p.vec_c,
              p.direct_epi, nsdb::gemm_kernel_name(p.kernel), p.kinter, nsdb::gemm_reducer_name(p.reducer),
              p.reduce_blocks, p.prefetch_eligible, p.packed, end);
}

int main() {
  nsdb::GemmCall c;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %d %lld %d %d", &c.M, &c.N, &c.K,
                    &c.batch, &c.splits, &c.cfg, &c.epi, &c.mfma, &c.fixup, &c.kinter, &c.out_f32, &c.accumulate,
                    &c.bias_mode, &c.lda, &c.ldb, &c.ldc, &c.sC, &c.c_align, &c.seg_k, &c.has_ws, &c.packed) == 21) {
    show(nsdb::gemm_plan(c), " | ");
    c.packed = 0;
    show(nsdb::gemm_plan(c), "\n");
  }
  return 0;
}
