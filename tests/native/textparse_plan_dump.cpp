// Host driver of tests/test_textparse_plan.py: one call per stdin line ("nbytes nfields delimiter"), one TextPlan per
// stdout line as "name=value" pairs. Built with the host C++ compiler against textparse_plan.h alone.
#include <cstdio>

#include "textparse_plan.h"

int main() {
  long long nbytes;
  int nfields, delim;
  while (std::scanf("%lld %d %d", &nbytes, &nfields, &delim) == 3) {
    const nsdb::TextPlan p = nsdb::textparse_plan(nbytes, nfields, delim);
    std::printf("rc=%d tile=%d tiles=%lld scan_step=%d launches=%d counts_bytes=%lld state_bytes=%lld "
                "scratch_bytes=%lld rows_bytes_1000=%lld flags_bytes_10=%lld\n",
                p.rc, p.tile, p.tiles, p.scan_step, p.launches, p.counts_bytes, p.state_bytes, p.scratch_bytes,
                nsdb::textparse_rows_bytes(1000), nsdb::textparse_flags_bytes(10));
  }
  return 0;
}
