// Prints the plans of relops_plan.h, one line of key=value words per request line read from stdin:
//   agg n F low_threshold mid want_inv want_first     aggwork n F pbits
//   call n F phase have_inv have_part_buffers vrs vcs (want_inv = 1, automatic threshold, MID on)
//   join n cap_override bloom_on min_bytes max_bytes part_on
//   jpart n cap filter bshift      part n P      tiles n      consts
// Built by tests/test_relops_plan.py with the host compiler alone.
#include <cstdio>
#include <cstring>

#include "relops_plan.h"

using namespace nsdb;

#define KV(name, v) std::printf(" " name "=%lld", (long long)(v))

static void dump_work(const AggWork& w) {
  KV("hist", w.hist); KV("tot", w.tot); KV("bstart", w.bstart); KV("pkey", w.pkey); KV("pval", w.pval);
  KV("prow", w.prow); KV("qkey", w.qkey); KV("qval", w.qval); KV("qrow", w.qrow); KV("end", w.end); KV("total", w.total);
}
static void dump_table(const char* pre, const AggTable& t) {
  const char* f[] = {"cap", "key", "acc", "cnt", "rmin", "gid", "words"};
  const long long v[] = {t.cap, t.key, t.acc, t.cnt, t.rmin, t.gid, t.words};
  for (int i = 0; i < 7; ++i) std::printf(" %s_%s=%lld", pre, f[i], v[i]);
}
static void dump_out(const char* pre, const AggOutLayout& o) {
  const char* f[] = {"ocap", "reps", "aggs", "cnt", "slot_of_gid", "first", "words"};
  const long long v[] = {o.ocap, o.reps, o.aggs, o.cnt, o.slot_of_gid, o.first, o.words};
  for (int i = 0; i < 7; ++i) std::printf(" %s_%s=%lld", pre, f[i], v[i]);
}
static void dump_jpart(const JoinPartPlan& p) {
  KV("rc", p.rc); KV("P", p.P); KV("G", p.G); KV("Pc", p.Pc); KV("sh", p.sh); KV("rpw", p.rpw); KV("staged", p.staged);
  KV("lds_hist", p.lds_hist); KV("hist", p.hist); KV("btot", p.btot); KV("cbase", p.cbase); KV("bbase", p.bbase);
  KV("ikey", p.ikey); KV("islot", p.islot); KV("irank", p.irank); KV("irow", p.irow); KV("ikey1", p.ikey1);
  KV("irow1", p.irow1); KV("end", p.end); KV("total", p.total);
}

int main() {
  char op[16];
  long long a[8];
  while (std::scanf("%15s", op) == 1) {
    auto need = [&](int k) {
      for (int i = 0; i < k; ++i)
        if (std::scanf("%lld", &a[i]) != 1) return false;
      return true;
    };
    if (!std::strcmp(op, "agg") && need(6)) {
      const AggPlan p = agg_plan(a[0], (int)a[1], a[2], a[3] != 0, a[4] != 0, a[5] != 0);
      KV("rc", p.rc); KV("rows", p.rows); KV("lcap_low", p.lcap_low); KV("lcap_part", p.lcap_part);
      KV("lcap_mid", p.lcap_mid); KV("low_thr", p.low_thr); KV("pbits", p.pbits); KV("P", p.P); KV("G", p.G);
      KV("rpw", p.rpw); KV("T", p.T); KV("T2", p.T2); KV("lds_low", p.lds_low); KV("lds_mid", p.lds_mid);
      KV("lds_hist", p.lds_hist); KV("lds_stage", p.lds_stage); KV("lds_bucket", p.lds_bucket);
      dump_table("glow", p.glow); dump_table("gpart", p.gpart); KV("ocap_low", p.ocap_low);
      dump_out("out1", agg_out(agg_ocap(p, 1), p.F)); dump_out("out2", agg_out(agg_ocap(p, 2), p.F));
      dump_work(p.work); KV("phase1_bytes", p.phase1_bytes); KV("part_bytes", p.part_bytes);
    } else if (!std::strcmp(op, "aggwork") && need(3)) {
      dump_work(agg_work(a[0], (int)a[1], (int)a[2]));
    } else if (!std::strcmp(op, "call") && need(7)) {
      KV("rc", agg_call_rc(agg_plan(a[0], (int)a[1], 0, true, true, true), (int)a[2], a[3] != 0, a[4] != 0, a[5], a[6]));
    } else if (!std::strcmp(op, "join") && need(6)) {
      const JoinPlan p = join_plan(a[0], a[1], a[2] != 0, a[3], a[4], a[5] != 0);
      KV("load", p.load); KV("cap", p.cap); KV("regions", p.regions); KV("part", p.part); KV("W", p.W);
      KV("bshift", p.bshift); KV("fold", p.fold);
      if (p.part) dump_jpart(p.work);
    } else if (!std::strcmp(op, "jpart") && need(4)) {
      dump_jpart(join_part_plan(a[0], a[1], a[2] != 0, (int)a[3]));
    } else if (!std::strcmp(op, "part") && need(2)) {
      const PartPlan p = part_plan(a[0], a[1]);
      KV("rc", p.rc); KV("G", p.G); KV("rpw", p.rpw); KV("lds_hist", p.lds_hist); KV("lds_scatter", p.lds_scatter);
      KV("hist", p.hist); KV("tot", p.tot); KV("bstart", p.bstart); KV("end", p.end); KV("total", p.total);
    } else if (!std::strcmp(op, "tiles") && need(1)) {
      KV("join_tiles", join_tiles(a[0])); KV("compact_tiles", compact_tiles(a[0]));
    } else if (!std::strcmp(op, "consts")) {
      KV("kSample", kSample); KV("kMetaStructWords", kMetaStructWords); KV("kMetaWords", kMetaWords);
      KV("kMidPMax", kMidPMax); KV("kLdsLow", kLdsLow); KV("kLdsPart", kLdsPart); KV("kLdsMid", kLdsMid);
      KV("kJRegionBits", kJRegionBits); KV("kJRegion", kJRegion); KV("kJWholeWrap", kJWholeWrap);
      KV("kJPartMaxRegions", kJPartMaxRegions); KV("kJPartOneLevel", kJPartOneLevel); KV("kJPartCoarse", kJPartCoarse);
      KV("kJStageBins", kJStageBins); KV("kJTile", kJTile); KV("kCompactTile", kCompactTile); KV("kTakeCols", kTakeCols);
    } else {
      std::fprintf(stderr, "bad request %s\n", op);
      return 2;
    }
    std::printf("\n");
  }
  return 0;
}
