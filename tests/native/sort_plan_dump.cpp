// Host driver of tests/test_sort_plan.py: one call per stdin line ("m n dt0 dt1 dt2 dt3"), one SortPlan per stdout
// line as "name=value" pairs. Built with the host C++ compiler against sort_plan.h alone.
#include <cstdio>

#include "sort_plan.h"

int main() {
  int m, dt[4];
  long long n;
  while (std::scanf("%d %lld %d %d %d %d", &m, &n, &dt[0], &dt[1], &dt[2], &dt[3]) == 6) {
    const nsdb::SortPlan p = nsdb::sort_plan(dt, m, n);
    std::printf("rc=%d word_bits=%d tile=%d tiles=%lld passes=%d launches=%d scan_step=%d hist_grid=%d "
                "state_bytes=%lld counts_bytes=%lld words_bytes=%lld ids_bytes=%lld scratch_bytes=%lld\n",
                p.rc, p.word_bits, p.tile, p.tiles, p.passes, p.launches, p.scan_step, p.hist_grid, p.state_bytes,
                p.counts_bytes, p.words_bytes, p.ids_bytes, p.scratch_bytes);
  }
  return 0;
}
