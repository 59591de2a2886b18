// Host plan of the relational operators (relops.hip): plain C++17, no HIP, so the host compiler alone builds it
// (tests/native/relops_plan_dump.cpp). Everything about a group-by, a join build or a partition that depends only on
// the call shape is decided here, once: table capacities, launch geometry, LDS bytes and the layout of every scratch
// buffer. The launchers take their pointers from these offsets and the binding sizes every allocation from the same
// plan. Nothing here depends on the data.
#pragma once

namespace nsdb {

typedef long long pl_i64;

constexpr pl_i64 pl_align16(pl_i64 b) { return (b + 15) & ~15LL; }
constexpr bool pl_pow2(pl_i64 x) { return x > 0 && (x & (x - 1)) == 0; }
inline pl_i64 pow2_at_least(pl_i64 x) {
  pl_i64 c = 1;
  while (c < x) c <<= 1;
  return c;
}
inline pl_i64 pow2_at_most(pl_i64 x) {
  pl_i64 c = 1;
  while (c * 2 <= x) c <<= 1;
  return c;
}

// ---------------------------------------------------------------- group-by
constexpr int kSample = 4096;   // rows of the distinct-key sample
// AggMeta (relops.hip) as int64 words: the struct, then the kSample sampled keys
enum AggMetaWord {
  kMetaEst = 0, kMetaLow, kMetaNgLow, kMetaNgPart, kMetaFailLow, kMetaFailPart, kMetaSentinelLow, kMetaSentinelPart,
  kMetaOccLow, kMetaOccPart, kMetaLowP, kMetaStructWords = 16
};
constexpr int kMetaWords = kMetaStructWords + kSample;
constexpr pl_i64 agg_entry_bytes(pl_i64 F) { return 20 + 8 * F; }   // LDS table entry [key | acc F | ref | rmin | cnt]
constexpr pl_i64 agg_stage_bytes(pl_i64 F) { return 14 + 8 * F; }   // staged row of a scatter pass
// LDS budgets: LOW <= 64 KiB (two workgroups per CU), PART <= 128 KiB, MID one CU's 160 KiB
constexpr pl_i64 kLdsLow = 64 * 1024, kLdsPart = 128 * 1024, kLdsMid = 160 * 1024;
// MID path: at most this many key partitions. Every workgroup of a row group reads all of its rows' keys through its
// own CU, so the per-CU load stream grows with P: measured (profiles/r5_relops) 16 M rows, 10 k keys at P = 5 took
// 0.65 ms against the PART path's 0.47, so MID stops at P = 3 (~6 k groups).
constexpr int kMidPMax = 3;

// rows staged per scatter pass of a 1024-thread workgroup: a multiple of 256 in [256, 4096], staging <= 96 KiB
inline int stage_rows(int F) {
  const int t = (int)(96 * 1024 / agg_stage_bytes(F)) / 256 * 256;   // wide rows (F up to 16): below one row per thread
  return t < 256 ? 256 : (t > 4096 ? 4096 : t);
}
// histogram / scatter workgroups (one per CU at most), >= 16 Ki rows each
inline int row_groups(pl_i64 n, int most) {
  const pl_i64 g = (n + 16383) / 16384;
  return (int)(g < 1 ? 1 : (g > most ? most : g));
}

// One open-addressing global table of cap + 1 slots, in u64 words: [key | acc F | cnt | rmin | gid_of_slot]
struct AggTable {
  pl_i64 cap, key, acc, cnt, rmin, gid, words;
};
inline AggTable agg_table(pl_i64 cap, int F) {
  const pl_i64 s = cap + 1;
  return {cap, 0, s, s + s * F, s + s * F + s, s + s * F + 2 * s, s * (4 + F)};
}
// The output buffer of a run that may create ocap groups, in i64 words: [reps | aggs F | cnt | slot_of_gid | first].
// slot_of_gid is written by nothing; dropping it would change the scratch bytes hash_aggregate reports.
struct AggOutLayout {
  pl_i64 ocap, reps, aggs, cnt, slot_of_gid, first, words;
};
inline AggOutLayout agg_out(pl_i64 ocap, int F) {
  return {ocap, 0, ocap, ocap * (1 + F), ocap * (2 + F), ocap * (3 + F), ocap * (4 + F)};
}
// The PART work buffer, in bytes: [hist P*G u32 | tot P | bstart P+2 | pkey n | pval n*F | prow n i32 | qkey | qval | qrow]
struct AggWork {
  pl_i64 hist, tot, bstart, pkey, pval, prow, qkey, qval, qrow, end, total;
};
inline AggWork agg_work(pl_i64 n, int F, int pbits) {
  const pl_i64 P = 1LL << pbits, G = row_groups(n, 256);
  AggWork w{};
  w.tot = pl_align16(P * G * 4);
  w.bstart = w.tot + 8 * P;
  w.pkey = w.bstart + 8 * (P + 2);
  w.pval = w.pkey + 8 * n;
  w.prow = w.pval + 8 * n * F;
  w.qkey = pl_align16(w.prow + 4 * n);
  w.qval = w.qkey + 8 * n;
  w.qrow = w.qval + 8 * n * F;
  w.end = w.qrow + 4 * n;
  w.total = w.tot + 8 * (2 * P + 2) + 2 * (8 * n + 8 * n * F + 4 * (n + 1)) + 64;
  return w;
}

enum {
  AGG_OK = 0, AGG_BAD_MID = -1, AGG_BAD_N = -2, AGG_BAD_F = -3, AGG_BAD_CAP = -4, AGG_BAD_LDS = -5, AGG_BAD_STAGE = -6,
  // the call, not the shape (agg_call_rc)
  AGG_BAD_PHASE = -7, AGG_NO_INV = -8, AGG_NO_PART_BUFFERS = -9, AGG_BAD_STRIDE = -10
};

struct AggPlan {
  int rc;                 // AGG_OK or the first failed check
  pl_i64 n;
  int F, want_inv, rows;  // rows: row ids travel through the partition passes (want_inv or want_first)
  int lcap_low, lcap_part, lcap_mid;   // LDS table slots; lcap_mid 0: no MID path
  int low_thr;            // largest estimated group count for the LOW path
  int pbits, P, G;        // PART: level-1 buckets, histogram / scatter workgroups
  pl_i64 rpw;             // rows per workgroup, even: every workgroup's key range starts 16-byte aligned
  int T, T2;              // rows staged per level-1 scatter pass / per sub-partition pass of the bucket kernel
  pl_i64 lds_low, lds_mid, lds_hist, lds_stage, lds_bucket;
  AggTable glow, gpart;
  pl_i64 ocap_low;        // groups phase 1 may create: the LOW table's slots, or every row
  AggWork work;
  pl_i64 phase1_bytes;    // meta + LOW table + inverse + the ocap_low output
  pl_i64 part_bytes;      // what the PART path adds: its table, the n-group output and the work buffer
};

// low_threshold > 0 pins the LOW / PART boundary (and so disables MID, like mid_enabled = false).
inline AggPlan agg_plan(pl_i64 n, int F, pl_i64 low_threshold, bool mid_enabled, bool want_inv, bool want_first) {
  AggPlan p{};
  p.n = n;
  p.F = F;
  p.want_inv = want_inv;
  p.rows = want_inv || want_first;
  const pl_i64 entry = agg_entry_bytes(F);
  // PART: level-1 buckets = one per CU (256) once there are >= 2048 rows per bucket; each bucket workgroup splits its
  // bucket further on the device from the sampled estimate, so no host decision needs the data
  p.lcap_low = (int)(entry > 0 ? pow2_at_most(kLdsLow / entry) : 1);
  if (p.lcap_low > 1024) p.lcap_low = 1024;   // <= 36 KB: 4+ LOW workgroups per CU
  p.lcap_part = (int)(entry > 0 ? pow2_at_most(kLdsPart / entry) : 1);
  if (p.lcap_part > 4096) p.lcap_part = 4096;
  // MID (agg_low_kernel MODE 2): up to kMidPMax hash partitions of the key space, each one CU-sized LDS table of
  // lcap_mid slots, half full at most. The LOW global table holds every MID group (sized for 8 partitions).
  if (mid_enabled && low_threshold <= 0) {
    p.lcap_mid = (int)(entry > 0 ? pow2_at_most(kLdsMid / entry) : 1);
    if (p.lcap_mid > 4096) p.lcap_mid = 4096;
  }
  const pl_i64 gcap_low = 4LL * p.lcap_low > 8LL * p.lcap_mid ? 4LL * p.lcap_low : 8LL * p.lcap_mid;
  // overflow table of the PART path (keys whose LDS probe window filled): a miss-sized estimate only
  pl_i64 gcap_part = n > 0 && n < (1LL << 31) ? pow2_at_least(2 * n) : 4096;
  gcap_part = gcap_part < 4096 ? 4096 : (gcap_part > (1LL << 17) ? 1LL << 17 : gcap_part);
  p.low_thr = (int)(low_threshold > 0 ? low_threshold : p.lcap_low / 4);
  while (p.pbits < 8 && n > 0 && (n >> (p.pbits + 1)) >= 2048) ++p.pbits;

  auto fail = [&p](int rc) {
    p.rc = rc;
    return p;
  };
  // the MID table fits one CU's LDS; the global table holds every MID group
  if (p.lcap_mid > 0 && (!pl_pow2(p.lcap_mid) || entry <= 0 || p.lcap_mid * entry > kLdsMid ||
                         gcap_low < 2LL * kMidPMax * (p.lcap_mid / 2)))
    return fail(AGG_BAD_MID);
  if (n < 1 || n >= (1LL << 31)) return fail(AGG_BAD_N);
  if (F < 0 || F > 16) return fail(AGG_BAD_F);
  if (!pl_pow2(gcap_low) || !pl_pow2(gcap_part) || !pl_pow2(p.lcap_low) || !pl_pow2(p.lcap_part)) return fail(AGG_BAD_CAP);
  if (p.lcap_low * entry > kLdsLow || p.lcap_part * entry > kLdsPart) return fail(AGG_BAD_LDS);
  p.T = stage_rows(F);
  p.T2 = p.T < 2048 ? p.T : 2048;   // 2 rows / thread
  if (p.T * agg_stage_bytes(F) > kLdsPart) return fail(AGG_BAD_STAGE);

  p.P = 1 << p.pbits;
  p.G = row_groups(n, 256);
  p.rpw = (((n + p.G - 1) / p.G) + 1) & ~1LL;
  p.lds_low = p.lcap_low * entry;
  p.lds_mid = p.lcap_mid * entry;
  p.lds_hist = 4LL * p.P;
  p.lds_stage = p.T * agg_stage_bytes(F);
  const pl_i64 sub = p.T2 * agg_stage_bytes(F), tab = p.lcap_part * entry;
  p.lds_bucket = sub > tab ? sub : tab;
  p.glow = agg_table(gcap_low, F);
  p.gpart = agg_table(gcap_part, F);
  p.ocap_low = n < gcap_low + 1 ? n : gcap_low + 1;
  p.work = agg_work(n, F, p.pbits);
  p.phase1_bytes = 8 * (kMetaWords + p.glow.words + (want_inv ? n : 0) + agg_out(p.ocap_low, F).words);
  p.part_bytes = 8 * (p.gpart.words + agg_out(n, F).words) + p.work.total;
  return p;
}

// groups the output buffer of a phase holds: 1 (sample + LOW) and 3 (LOW emit) run on the small one
inline pl_i64 agg_ocap(const AggPlan& p, int phase) { return phase == 1 || phase == 3 ? p.ocap_low : p.n; }

// The checks of one launch that depend on the call rather than the shape. Phases: 0 everything, 1 init + sample +
// LOW, 2 PART, 3 emit + inverse fix-up.
inline int agg_call_rc(const AggPlan& p, int phase, bool have_inv, bool have_part_buffers, pl_i64 vrs, pl_i64 vcs) {
  if (p.rc != AGG_OK) return p.rc;
  if (phase < 0 || phase > 3) return AGG_BAD_PHASE;
  if (p.want_inv && !have_inv) return AGG_NO_INV;
  if ((phase == 0 || phase == 2) && !have_part_buffers) return AGG_NO_PART_BUFFERS;
  if (p.F > 0 && (vrs < 0 || vcs < 0)) return AGG_BAD_STRIDE;
  return AGG_OK;
}

// ---------------------------------------------------------------- hash join
// Tables of more than kJWholeWrap slots probe linearly inside aligned regions of kJRegion slots (a chain wraps at its
// region's end) and are built region by region in LDS; smaller ones (builds up to ~1 M rows, whose table fits the
// MALL) probe the whole table with plain linear probing and take the global-atomic insert. Every probe
// (join_probe_kernel, pipeline_core.h join_find / join_find_rows) walks the same order.
constexpr int kJRegionBits = 12;
constexpr unsigned long long kJRegion = 1ull << kJRegionBits;
constexpr unsigned long long kJWholeWrap = 1ull << 22;   // tables of at most this many slots: chains wrap at the table's end
// Partitioned build (tables of 2..kJPartMaxRegions regions). Up to kJPartOneLevel regions the rows are partitioned
// straight into regions; beyond, into kJPartCoarse coarse bins first (sh = log2 of the regions per coarse bin), then
// split per coarse bin. A coarse scatter of at most kJStageBins bins is staged through LDS.
constexpr long long kJPartMaxRegions = 8192;
constexpr unsigned kJPartOneLevel = 2048, kJPartCoarse = 256;
constexpr int kJStageBins = 1024;
constexpr int kJTile = 4096;        // probe rows per workgroup tile (256 threads x 16)
constexpr int kCompactTile = 8192;  // rows per compaction / run-count tile (one 256-thread workgroup)
constexpr int kTakeCols = 48;       // columns one take_many launch gathers

inline pl_i64 join_tiles(pl_i64 m) { return (m + kJTile - 1) / kJTile; }
inline pl_i64 compact_tiles(pl_i64 n) { return (n + kCompactTile - 1) / kCompactTile; }

// log2(slots per filter word) of a W-word probe filter over cap slots (both powers of two, W <= cap)
inline int join_filter_shift(pl_i64 cap, pl_i64 W) {
  int sh = 0;
  while ((W << sh) < cap) ++sh;
  return sh;
}
// a filter word covers 4..kJRegion slots: the region pass writes it with its region
constexpr bool join_filter_folds(int bshift) { return bshift >= 2 && bshift <= kJRegionBits; }

enum {
  JOIN_OK = 0, JOIN_BAD_N = -1, JOIN_NOT_REGIONS = -2, JOIN_CAP_NOT_POW2 = -3, JOIN_CAP_SMALL = -4, JOIN_CAP_LARGE = -5,
  JOIN_TOO_MANY_REGIONS = -6, JOIN_BAD_FILTER = -7
};

// Workspace of the partitioned build, in bytes: [hist (Pc+1)*G u32 | btot Pc+1 | cbase Pc+2 | bbase P+2 | ikey n |
// islot n i32 | irank n u32 | irow n u32 | two-level only: ikey1 n | irow1 n u32]
struct JoinPartPlan {
  int rc;
  unsigned P, G, Pc;      // regions, histogram / scatter workgroups, first-level bins (P >> sh)
  int sh;                 // 0: one level
  pl_i64 rpw;
  bool staged;            // the coarse scatter goes through LDS
  pl_i64 lds_hist;
  pl_i64 hist, btot, cbase, bbase, ikey, islot, irank, irow, ikey1, irow1, end, total;
};
// filter: the region pass also writes a probe filter of shift bshift. rc: JOIN_OK or the first failed check.
inline JoinPartPlan join_part_plan(pl_i64 n, pl_i64 cap, bool filter, int bshift) {
  JoinPartPlan p{};
  p.P = (unsigned)(cap >> kJRegionBits);
  p.G = (unsigned)row_groups(n, 1024);
  p.rpw = (n + p.G - 1) / p.G;
  if (p.P > kJPartOneLevel)
    while ((p.P >> p.sh) > kJPartCoarse) ++p.sh;
  p.Pc = p.P >> p.sh;
  p.staged = p.sh && p.Pc + 1 <= (unsigned)kJStageBins;
  p.lds_hist = 4LL * (p.Pc + 1);
  const pl_i64 hist = pl_align16(4LL * (p.Pc + 1) * p.G);
  p.btot = hist;
  p.cbase = p.btot + 8LL * (p.Pc + 1);
  p.bbase = p.cbase + 8LL * (p.Pc + 2);
  p.ikey = pl_align16(p.bbase + 8LL * (p.P + 2));
  p.islot = p.ikey + 8 * n;
  p.irank = p.islot + 4 * n;
  p.irow = p.irank + 4 * n;
  p.end = p.irow + 4 * n;
  if (p.sh) {
    p.ikey1 = pl_align16(p.end);
    p.irow1 = p.ikey1 + 8 * n;
    p.end = p.irow1 + 4 * n;
  } else {   // one level: the scatter writes the region items themselves
    p.ikey1 = p.ikey;
    p.irow1 = p.irow;
  }
  p.total = hist + 8LL * (p.Pc + 1) + 8LL * (p.Pc + 2) + 8LL * (p.P + 2) + n * 20 + (p.sh ? n * 12 : 0) + 64;
  // the layout above holds for any n and cap; the launcher takes only these
  if (n <= 0) p.rc = JOIN_BAD_N;
  else if (cap <= (pl_i64)kJWholeWrap) p.rc = JOIN_NOT_REGIONS;
  else if (!pl_pow2(cap)) p.rc = JOIN_CAP_NOT_POW2;
  else if (cap < 2 * n) p.rc = JOIN_CAP_SMALL;
  else if (cap >= (1LL << 31)) p.rc = JOIN_CAP_LARGE;
  else if ((cap >> kJRegionBits) > kJPartMaxRegions) p.rc = JOIN_TOO_MANY_REGIONS;
  else if (filter && !join_filter_folds(bshift)) p.rc = JOIN_BAD_FILTER;
  return p;
}

struct JoinPlan {
  int load;               // slots per build row at least: 8 up to 2^18 rows, 4 up to 2^22, 2 beyond
  pl_i64 cap;             // slots (a power of two >= 1024); the table has cap + 1
  bool regions;           // chains wrap inside kJRegion-slot regions; the build reads back {fail, max count}
  bool part;              // built region by region in LDS (join_part_plan), else the global-atomic insert
  pl_i64 W;               // probe filter words, 0: none
  int bshift;             // log2(slots per filter word), -1: no filter
  bool fold;              // the region pass writes the filter
  JoinPartPlan work;      // part only
};
// Load factor: <= 1/8 for builds up to 256 k rows (a <= 64 MiB table: a probe of an ABSENT key — most probe rows of a
// selective join, TPC-H Q17's 60 M lineitems against ~2 k parts — expects ~1.1 slot reads instead of ~2.5 at 1/2),
// <= 1/4 up to 4 M rows, <= 1/2 beyond. cap_override > 0: a rebuild at that many slots.
// Probe filter: for tables past the L2 (more than bloom_min_bytes of slots), ~16 filter bits per build row, while the
// filter itself stays L2-sized (<= bloom_max_bytes). A larger one sits in the MALL next to the table, and its word is a
// second dependent far read for every probe that matches (16 M-row build, 90 % matching probes: 0.89 ms with the
// filter, 0.70 without, profiles/r6_join).
inline JoinPlan join_plan(pl_i64 n, pl_i64 cap_override, bool bloom_on, pl_i64 bloom_min_bytes, pl_i64 bloom_max_bytes,
                          bool part_on) {
  JoinPlan p{};
  p.load = n <= (1LL << 18) ? 8 : (n <= (1LL << 22) ? 4 : 2);
  p.cap = cap_override > 0 ? cap_override : pow2_at_least(p.load * n > 1024 ? p.load * n : 1024);
  p.regions = p.cap > (pl_i64)kJWholeWrap;
  p.part = p.regions && (p.cap >> kJRegionBits) <= kJPartMaxRegions && part_on;
  p.bshift = -1;
  const pl_i64 want = pow2_at_least((16 * n + 63) / 64 > 64 ? (16 * n + 63) / 64 : 64);
  const pl_i64 W = want < p.cap ? want : p.cap;
  if (bloom_on && p.cap * 16 > bloom_min_bytes && W * 8 <= bloom_max_bytes) {
    p.W = W;
    p.bshift = join_filter_shift(p.cap, W);
  }
  p.fold = p.part && join_filter_folds(p.bshift);
  if (p.part) p.work = join_part_plan(n, p.cap, p.fold, p.bshift);
  return p;
}

// ---------------------------------------------------------------- stable partition permutation
enum { PART_OK = 0, PART_BAD_P = -1, PART_BAD_N = -2, PART_BAD_LDS = -3 };
constexpr int kPartMaxP = 2048;

// work, in bytes: [hist P*G u32 | tot P i64 | bstart P+1 i64]
struct PartPlan {
  int rc;
  int G;
  pl_i64 rpw, lds_hist, lds_scatter;
  pl_i64 hist, tot, bstart, end, total;
};
inline PartPlan part_plan(pl_i64 n, pl_i64 P) {
  PartPlan p{};
  if (P <= 0 || P > kPartMaxP) p.rc = PART_BAD_P;
  else if (n < 1 || n >= (1LL << 31)) p.rc = PART_BAD_N;
  else if (P * 4 * 17 > kLdsMid) p.rc = PART_BAD_LDS;
  if (p.rc != PART_OK) return p;
  p.G = row_groups(n, 256);
  p.rpw = (n + p.G - 1) / p.G;
  p.lds_hist = P * 4;
  p.lds_scatter = P * 4 * 17;
  p.tot = pl_align16(P * p.G * 4);
  p.bstart = p.tot + 8 * P;
  p.end = p.bstart + 8 * (P + 1);
  p.total = p.tot + 8 * (2 * P + 1) + 64;
  return p;
}

}  // namespace nsdb
