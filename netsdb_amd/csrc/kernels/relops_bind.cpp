// PyTorch bindings of the device relational operators (relops.hip): hash aggregation, hash join build /
// probe, and the stable partition permutation of the shuffle sink. Every entry checks device / dtype / shape
// on the host before anything is launched, and launches on the current HIP stream.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <limits>
#include <string>
#include <tuple>
#include <vector>

#include "relops_plan.h"

typedef long long ll;
template <typename T> ll* LL(T* p) { return reinterpret_cast<ll*>(p); }

extern "C" {
int nsdb_hash_aggregate(const void* keys, const void* vals, long long n, int F, int vt, int op, int want_inv,
                        int want_first, long long low_threshold, int mid, void* meta, void* glow, void* gpart, void* out,
                        void* inv, int phase, void* work, long long vrs, long long vcs, hipStream_t st);
int nsdb_join_insert(const void* keys, long long n, void* tab, long long cap, int* row_slot, unsigned* row_rank,
                     unsigned long long* ndup, unsigned* fail, hipStream_t st);
int nsdb_join_build_part(const void* keys, long long n, void* tab, long long cap, void* work,
                         unsigned long long* ctr, unsigned long long* bloom, int bshift, long long* perm, hipStream_t st);
int nsdb_join_perm(const int* row_slot, const unsigned* row_rank, long long n, const unsigned long long* ndup,
                   unsigned long long* bump, void* tab, long long cap, long long* perm, hipStream_t st);
int nsdb_join_probe(const void* keys, long long m, const void* tab, long long cap, unsigned* cnt, unsigned* pay,
                    long long* tile_sum, const unsigned long long* bloom, int bshift, hipStream_t st);
int nsdb_join_bloom(const void* tab, long long cap, long long W, unsigned long long* bloom, hipStream_t st);
int nsdb_join_init(void* tab, long long cap, hipStream_t st);
int nsdb_take_many(const void* const* src, void* const* dst, const long long* nsrc, const int* w, const int* per,
                   int ncols, const long long* idx, long long n, int* bad, hipStream_t st);
int nsdb_join_expand(const unsigned* cnt, const unsigned* pay, long long m, const long long* tile_base,
                     const long long* perm, long long* bidx, long long* pidx, hipStream_t st);
int nsdb_mix64(const void* x, const void* y, void* out, long long n, hipStream_t st);
int nsdb_compact_count(const unsigned char* mask, long long n, unsigned* cnt, long long* off, hipStream_t st);
int nsdb_compact_write(const unsigned char* mask, long long n, const long long* off, long long* out, hipStream_t st);
int nsdb_partition_perm(const long long* dest, long long n, int P, void* work, long long* perm, long long* counts,
                        hipStream_t st);
int nsdb_run_count(const void* keys, long long n, unsigned* cnt, long long* off, hipStream_t st);
int nsdb_run_reduce(const void* keys, const void* vals, long long rs, long long cs, int F, int vt, int op, long long n,
                    const long long* off, long long G, long long* heads, long long* okey, void* oagg, long long* ocnt,
                    hipStream_t st);
int nsdb_order_limit_max_k();
long long nsdb_order_limit_state_bytes(const int* dt, int m, long long n);
int nsdb_order_limit(const void* const* keys, const int* dt, const int* desc, int m, long long n, long long k,
                     void* state, unsigned* lists, unsigned* win, long long* out, hipStream_t st);
int nsdb_order_by_tile();
int nsdb_order_by_plan(const int* dt, int m, long long n, long long* fields);
int nsdb_order_by(const void* const* keys, const int* dt, const int* desc, int m, long long n, long long limit,
                  void* state, void* counts, void* words, void* ids, long long* out, hipStream_t st);
}

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

bool g_agg_mid = true;   // the MID group-by path (agg_set_mid: A/B and tests)
bool g_join_bloom = true; // probe filters of large join tables (join_set_bloom: A/B and tests)
bool g_join_part = true;  // partitioned (LDS region) build of multi-region join tables (join_set_part: A/B and tests)
int64_t g_join_bloom_min_bytes = int64_t(4) << 20;   // ... of tables with more slot bytes than this (past the L2)
int64_t g_join_bloom_max_bytes = int64_t(4) << 20;   // ... whose filter has at most this many bytes

void rc_ok(int rc, const char* what) {
  TORCH_CHECK(rc == 0, what, " failed with code ", rc, " (", hipGetErrorString((hipError_t)(rc > 0 ? rc : 0)), ")");
}

int op_code(const std::string& op) {
  const int opc = op == "sum" ? 0 : op == "min" ? 1 : op == "max" ? 2 : -1;
  TORCH_CHECK(opc >= 0, "op must be sum, min or max");
  return opc;
}

// The value columns of a group-by: [n] or [n, F] float64 / int64 on the keys' device, or none (F = 0).
struct AggVals {
  torch::Tensor v;
  int F = 0, vt = 0;             // vt: 0 double, 1 int64
  int64_t vrs = 0, vcs = 0;      // element strides of a row / a column
  c10::ScalarType dtype = torch::kFloat64;
  const void* ptr() const { return F ? v.data_ptr() : nullptr; }
};
// in_place: row-major [n, F] or column-major (the transpose of a contiguous [F, n] stack) are read where they are,
// anything else is made contiguous; otherwise any strides are taken as they come
AggVals agg_vals(const c10::optional<torch::Tensor>& vals, const torch::Tensor& keys, bool in_place) {
  AggVals a;
  if (!vals.has_value() || !vals->defined() || vals->numel() == 0) return a;
  const int64_t n = keys.numel();
  a.v = *vals;
  TORCH_CHECK(a.v.is_cuda() && a.v.device() == keys.device(), "vals must be on the keys' device");
  TORCH_CHECK(a.v.scalar_type() == torch::kFloat64 || a.v.scalar_type() == torch::kInt64, "vals must be float64 or int64");
  if (a.v.dim() == 1) a.v = a.v.unsqueeze(1);
  TORCH_CHECK(a.v.dim() == 2 && a.v.size(0) == n, "vals must be [n] or [n, F]");
  a.vrs = a.v.stride(0);
  a.vcs = a.v.stride(1);
  if (in_place) {
    const bool colmajor = a.v.size(1) > 1 && a.v.stride(0) == 1 && a.v.stride(1) >= n;
    if (!colmajor) a.v = a.v.contiguous();
    a.vrs = a.v.size(1) > 1 ? a.v.stride(0) : 1;
    a.vcs = a.v.size(1) > 1 ? a.v.stride(1) : 1;
  }
  a.F = (int)a.v.size(1);
  a.vt = a.v.scalar_type() == torch::kInt64 ? 1 : 0;
  a.dtype = a.v.scalar_type();
  return a;
}

// Group n int64 keys and reduce F value columns per group on the device.
//   vals: [n, F] float64 or int64 (or None / F == 0: counts only); op: "sum" | "min" | "max".
// Returns (reps [g] i64, aggs [g, F] (vals dtype), counts [g] i64, first [g] i64 (smallest row of each group; only
// meaningful with want_first, which otherwise lets the partition passes skip row ids),
// inv [n] i64 (or empty), status): status = [g, path (0 LOW, 1 PART), ok (0: the PART table overflowed; outputs
// invalid, fall back), distinct keys in the 4096-row sample, scratch bytes used]. low_threshold: largest estimated
// group count for the LOW path (0: automatic).
//
// Every buffer is sized by agg_plan (relops_plan.h), for the path that runs. Phase 1 (sample + LOW) needs O(groups)
// words: the LOW global table and an output of ocap_low groups. Only when the device reports that the LOW path did not
// take the rows (one host read, which the LOW path needs anyway for its group count) are the PART buffers allocated —
// about 2 (12 + 8 F) n bytes of partitioned rows plus an n-group output — and `scratch(+bytes)` / `scratch(-bytes)` (a
// Python callable, e.g. the storage manager's device-budget accounting) is told before they are allocated and after
// they are released.
std::vector<torch::Tensor> hash_aggregate(torch::Tensor keys, c10::optional<torch::Tensor> vals, const std::string& op,
                                          bool want_inv, int64_t low_threshold, bool want_first,
                                          pybind11::object scratch) {
  TORCH_CHECK(keys.is_cuda(), "keys must be a GPU tensor");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64 && keys.dim() == 1, "keys must be 1-D int64");
  keys = keys.contiguous();
  const int64_t n = keys.numel();
  TORCH_CHECK(n < (int64_t(1) << 31), "hash_aggregate: at most 2^31 - 1 rows per call (the caller chunks)");
  const int opc = op_code(op);
  const AggVals a = agg_vals(vals, keys, true);
  const int F = a.F;
  TORCH_CHECK(F <= 16, "at most 16 value columns");
  auto i64 = keys.options().dtype(torch::kInt64);
  if (n == 0) {
    return {torch::empty({0}, i64), torch::empty({0, F}, keys.options().dtype(a.dtype)), torch::empty({0}, i64),
            torch::empty({0}, i64), torch::empty({0}, i64), torch::tensor({0, 0, 1, 0, 0}, torch::kInt64)};
  }
  const nsdb::AggPlan p = nsdb::agg_plan(n, F, low_threshold, g_agg_mid, want_inv, want_first);
  TORCH_CHECK(p.rc == nsdb::AGG_OK, "hash_aggregate: bad plan (code ", p.rc, ")");
  auto meta = torch::empty({nsdb::kMetaWords}, i64);
  auto glow = torch::empty({p.glow.words}, i64);
  auto inv = want_inv ? torch::empty({n}, i64) : torch::empty({0}, i64);
  auto out = torch::empty({nsdb::agg_out(p.ocap_low, F).words}, i64);
  auto launch = [&](int phase, void* gpart, void* work) {
    rc_ok(nsdb_hash_aggregate(keys.data_ptr(), a.ptr(), n, F, a.vt, opc, want_inv ? 1 : 0, want_first ? 1 : 0,
                              low_threshold, g_agg_mid ? 1 : 0, meta.data_ptr(), glow.data_ptr(), gpart, out.data_ptr(),
                              want_inv ? inv.data_ptr() : nullptr, phase, work, (long long)a.vrs, (long long)a.vcs,
                              stream()),
          "hash_aggregate");
  };
  auto read_meta = [&]() { return meta.narrow(0, 0, nsdb::kMetaStructWords).cpu(); };   // the host read: counts and flags
  launch(1, nullptr, nullptr);
  auto m = read_meta();
  const ll* mp = LL(m.data_ptr<int64_t>());
  const bool low_ok = mp[nsdb::kMetaLow] != 0 && mp[nsdb::kMetaFailLow] == 0;
  int64_t scratch_bytes = p.phase1_bytes;
  bool ok = true;
  int64_t g = 0;
  if (low_ok) {
    launch(3, nullptr, nullptr);
    g = (int64_t)mp[nsdb::kMetaNgLow];
  } else {
    if (!scratch.is_none()) scratch(p.part_bytes);
    try {
      auto gpart = torch::empty({p.gpart.words}, i64);
      auto work = torch::empty({(p.work.total + 7) / 8}, i64);
      out = torch::empty({nsdb::agg_out(n, F).words}, i64);
      launch(2, gpart.data_ptr(), work.data_ptr());
      auto m2 = read_meta();
      const ll* mp2 = LL(m2.data_ptr<int64_t>());
      g = (int64_t)mp2[nsdb::kMetaNgPart];
      ok = mp2[nsdb::kMetaFailPart] == 0;
      scratch_bytes += p.part_bytes - 8 * nsdb::agg_out(p.ocap_low, F).words;
    } catch (...) {
      if (!scratch.is_none()) scratch(-p.part_bytes);
      throw;
    }
    if (!scratch.is_none()) scratch(-p.part_bytes);
  }
  auto status = torch::tensor({(int64_t)g, (int64_t)(low_ok ? 0 : 1), (int64_t)(ok ? 1 : 0), (int64_t)mp[nsdb::kMetaEst],
                               scratch_bytes}, torch::kInt64);
  if (!ok) return {torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), status};
  const nsdb::AggOutLayout o = nsdb::agg_out(low_ok ? p.ocap_low : n, F);
  auto reps = out.narrow(0, o.reps, g);
  auto aggs = out.narrow(0, o.aggs, g * F).view({g, F});
  if (a.vt == 0) aggs = aggs.view(torch::kFloat64);
  auto cnt = out.narrow(0, o.cnt, g);
  auto first = out.narrow(0, o.first, g);
  // the views keep the whole ocap-row buffer alive: copy small results out of a large one
  if (o.ocap > p.ocap_low && g * 4 < o.ocap) {
    reps = reps.clone();
    aggs = aggs.clone();
    cnt = cnt.clone();
    first = first.clone();
  }
  return {reps, aggs, cnt, first, inv, status};
}

nsdb::JoinPlan join_plan_now(int64_t n, int64_t cap_override) {
  return nsdb::join_plan(n, cap_override, g_join_bloom, g_join_bloom_min_bytes, g_join_bloom_max_bytes, g_join_part);
}

// Join build: returns (table [cap+1, 2] i64 of 16-byte slots {key, cnt | pay << 32}, perm [n] i64: the CSR runs of
// repeated keys; untouched when no key repeats, every payload being the build row itself). No host read.
// join_plan (relops_plan.h) decides the load factor, the table kind, the probe filter and the workspace. A region
// table is built region by region in LDS and checked once on the host for a region left without an empty slot (a hash
// pile-up far outside the load's statistics), in which case it doubles and is rebuilt. Smaller ones: the global
// insert, whole-table linear probing.
std::vector<torch::Tensor> join_build(torch::Tensor keys) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64 && keys.dim() == 1, "keys: 1-D int64 GPU tensor");
  keys = keys.contiguous();
  const int64_t n = keys.numel();
  TORCH_CHECK(n < (int64_t(1) << 29), "join_build: at most 2^29 build rows per table");
  auto i64 = keys.options().dtype(torch::kInt64);
  int64_t cap_override = 0;
  for (int attempt = 0;; ++attempt) {
    const nsdb::JoinPlan p = join_plan_now(n, cap_override);
    const int64_t cap = p.cap;
    auto tab = torch::empty({cap + 1, 2}, i64);
    auto ctr = torch::zeros({3}, i64);   // [repeated-key rows, run bump counter, fail]
    auto* c = reinterpret_cast<unsigned long long*>(ctr.data_ptr<int64_t>());
    auto perm = torch::empty({n}, i64);
    auto bloom = torch::empty({p.W}, i64);
    auto* bp = reinterpret_cast<unsigned long long*>(bloom.data_ptr<int64_t>());
    if (p.part) {
      TORCH_CHECK(p.work.rc == nsdb::JOIN_OK, "join_build: bad plan (code ", p.work.rc, ")");
      auto work = torch::empty({(p.work.total + 7) / 8}, i64);
      rc_ok(nsdb_join_build_part(keys.data_ptr(), n, tab.data_ptr(), cap, work.data_ptr(), c, p.fold ? bp : nullptr,
                                 p.bshift, LL(perm.data_ptr<int64_t>()), stream()),
            "join_build_part");
    } else {
      rc_ok(nsdb_join_init(tab.data_ptr(), cap, stream()), "join_init");
      auto row_slot = torch::empty({n}, keys.options().dtype(torch::kInt32));
      auto row_rank = torch::empty({n}, keys.options().dtype(torch::kInt32));
      rc_ok(nsdb_join_insert(keys.data_ptr(), n, tab.data_ptr(), cap, row_slot.data_ptr<int>(),
                             reinterpret_cast<unsigned*>(row_rank.data_ptr<int>()), c,
                             reinterpret_cast<unsigned*>(c + 2), stream()),
            "join_insert");
      // the table keeps each key's EXTRA-row count (join_probe adds the claiming row)
      rc_ok(nsdb_join_perm(row_slot.data_ptr<int>(), reinterpret_cast<const unsigned*>(row_rank.data_ptr<int>()), n, c,
                           c + 1, tab.data_ptr(), cap, LL(perm.data_ptr<int64_t>()), stream()),
            "join_perm");
    }
    if (p.W > 0 && !p.fold) {
      bloom.zero_();
      rc_ok(nsdb_join_bloom(tab.data_ptr(), cap, p.W, bp, stream()), "join_bloom");
    }
    // Region tables (builds past ~1 M rows) read {fail, largest extra-row count} in one transfer: a region left
    // without an empty slot is rebuilt larger; the count is the table's max multiplicity - 1 (JoinTable
    // .max_multiplicity, which sizes the fused probes' output regions, needs no read of its own). Whole-table tables
    // cannot fill (load <= 1/2): no host read.
    torch::Tensor stat = torch::empty({0}, i64);
    if (p.regions) {
      stat = torch::stack({ctr[2], tab.select(1, 1).bitwise_and(0xFFFFFFFFLL).max()}).cpu();
      if (stat[0].item<int64_t>() != 0) {                    // a region without an empty slot: rebuild larger
        TORCH_CHECK(attempt < 2 && cap * 2 < (int64_t(1) << 31),
                    "join_build: hash regions overflow even at ", cap, " slots for ", n, " rows");
        cap_override = cap * 2;
        continue;
      }
    }
    return {tab, perm, bloom, stat};
  }
}

// bloom: the table's probe filter from join_build (empty: none); shift = log2(slots per filter word)
int bloom_shift(const torch::Tensor& tab, const c10::optional<torch::Tensor>& bloom) {
  if (!bloom.has_value() || !bloom->defined() || bloom->numel() == 0) return -1;
  const int64_t cap = tab.size(0) - 1, W = bloom->numel();
  TORCH_CHECK(W <= cap && (W & (W - 1)) == 0 && bloom->is_contiguous() && bloom->scalar_type() == torch::kInt64 &&
                  bloom->device() == tab.device(), "malformed join probe filter");
  return nsdb::join_filter_shift(cap, W);
}

// Probe a built table with m int64 keys: all (build row, probe row) pairs with equal keys, probe-major.
std::vector<torch::Tensor> join_probe(torch::Tensor tab, torch::Tensor perm, torch::Tensor keys,
                                      c10::optional<torch::Tensor> bloom) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64 && keys.dim() == 1, "keys: 1-D int64 GPU tensor");
  TORCH_CHECK(tab.is_cuda() && tab.scalar_type() == torch::kInt64 && tab.dim() == 2 && tab.size(1) == 2 &&
                  tab.is_contiguous() && perm.scalar_type() == torch::kInt64,
              "join table tensors (from join_build) expected");
  const int64_t cap = tab.size(0) - 1;
  TORCH_CHECK(cap >= 1024 && (cap & (cap - 1)) == 0, "malformed join table");
  TORCH_CHECK(keys.device() == tab.device(), "probe keys must be on the table's device");
  keys = keys.contiguous();
  const int64_t m = keys.numel();
  auto i64 = keys.options().dtype(torch::kInt64);
  if (m == 0) return {torch::empty({0}, i64), torch::empty({0}, i64)};   // (an empty perm: unique build keys)
  auto i32 = keys.options().dtype(torch::kInt32);
  auto cnt = torch::empty({m}, i32);
  auto pay = torch::empty({m}, i32);
  const int64_t tiles = nsdb::join_tiles(m);
  auto tsum = torch::empty({tiles + 1}, i64);
  const int bsh = bloom_shift(tab, bloom);
  rc_ok(nsdb_join_probe(keys.data_ptr(), m, tab.data_ptr(), cap, reinterpret_cast<unsigned*>(cnt.data_ptr<int>()),
                        reinterpret_cast<unsigned*>(pay.data_ptr<int>()), LL(tsum.data_ptr<int64_t>()),
                        bsh >= 0 ? reinterpret_cast<const unsigned long long*>(bloom->data_ptr<int64_t>()) : nullptr,
                        bsh, stream()),
        "join_probe");
  auto incl = torch::cumsum(tsum.narrow(0, 0, tiles), 0);
  const int64_t total = incl[tiles - 1].item<int64_t>();   // sizes the output (one host read)
  auto base = incl.sub_(tsum.narrow(0, 0, tiles));
  auto bidx = torch::empty({total}, i64);
  auto pidx = torch::empty({total}, i64);
  if (total > 0)
    rc_ok(nsdb_join_expand(reinterpret_cast<const unsigned*>(cnt.data_ptr<int>()),
                           reinterpret_cast<const unsigned*>(pay.data_ptr<int>()), m, LL(base.data_ptr<int64_t>()),
                           LL(perm.data_ptr<int64_t>()), LL(bidx.data_ptr<int64_t>()), LL(pidx.data_ptr<int64_t>()),
                           stream()),
          "join_expand");
  return {bidx, pidx};
}

// Stable partition permutation of dest (values in [0, P)): rows of partition 0 first (input order), then 1, ...
std::vector<torch::Tensor> partition_perm(torch::Tensor dest, int64_t P) {
  TORCH_CHECK(dest.is_cuda() && dest.scalar_type() == torch::kInt64 && dest.dim() == 1, "dest: 1-D int64 GPU tensor");
  TORCH_CHECK(P >= 1 && P <= nsdb::kPartMaxP, "partition_perm: 1 <= P <= ", nsdb::kPartMaxP);
  dest = dest.contiguous();
  const int64_t n = dest.numel();
  TORCH_CHECK(n < (int64_t(1) << 31), "partition_perm: at most 2^31 - 1 rows");
  auto i64 = dest.options().dtype(torch::kInt64);
  auto counts = torch::zeros({P}, i64);
  auto perm = torch::empty({n}, i64);
  if (n == 0) return {perm, counts};
  auto work = torch::empty({(nsdb::part_plan(n, P).total + 7) / 8}, i64);
  rc_ok(nsdb_partition_perm(LL(dest.data_ptr<int64_t>()), n, (int)P, work.data_ptr(), LL(perm.data_ptr<int64_t>()),
                            LL(counts.data_ptr<int64_t>()), stream()),
        "partition_perm");
  return {perm, counts};
}

// Row ids of the set rows of a 0/1 byte mask (bool or uint8), in order: torch.nonzero(mask).flatten() as three
// streaming launches + one read of the total (the output size).
torch::Tensor compact(torch::Tensor mask) {
  TORCH_CHECK(mask.is_cuda() && mask.dim() == 1 && (mask.scalar_type() == torch::kBool ||
                                                     mask.scalar_type() == torch::kUInt8),
              "compact: 1-D bool / uint8 GPU mask");
  mask = mask.contiguous();
  const int64_t n = mask.numel();
  auto i64 = mask.options().dtype(torch::kInt64);
  if (n == 0) return torch::empty({0}, i64);
  const unsigned char* mp = reinterpret_cast<const unsigned char*>(mask.data_ptr());
  if (reinterpret_cast<uintptr_t>(mp) & 15) {
    mask = mask.clone();
    mp = reinterpret_cast<const unsigned char*>(mask.data_ptr());
  }
  const int64_t T = nsdb::compact_tiles(n);
  auto cnt = torch::empty({T}, mask.options().dtype(torch::kInt32));
  auto off = torch::empty({T + 1}, i64);
  rc_ok(nsdb_compact_count(mp, n, reinterpret_cast<unsigned*>(cnt.data_ptr<int32_t>()), LL(off.data_ptr<int64_t>()),
                           stream()),
        "compact_count");
  const int64_t total = off[T].item<int64_t>();
  auto out = torch::empty({total}, i64);
  if (total > 0)
    rc_ok(nsdb_compact_write(mp, n, LL(off.data_ptr<int64_t>()), LL(out.data_ptr<int64_t>()), stream()),
          "compact_write");
  return out;
}

// mix64((x ^ y) + GOLD) per row (y optional), int64 in / out: the engine's key hash in one pass.
torch::Tensor mix64(torch::Tensor x, c10::optional<torch::Tensor> y) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kInt64 && x.dim() == 1, "mix64: x must be a 1-D int64 GPU tensor");
  x = x.contiguous();
  const void* yp = nullptr;
  torch::Tensor yc;
  if (y.has_value() && y->defined()) {
    TORCH_CHECK(y->is_cuda() && y->scalar_type() == torch::kInt64 && y->numel() == x.numel() && y->device() == x.device(),
                "mix64: y must be an int64 GPU tensor like x");
    yc = y->contiguous();
    yp = yc.data_ptr();
  }
  auto out = torch::empty_like(x);
  const bool aligned = ((reinterpret_cast<uintptr_t>(x.data_ptr()) | reinterpret_cast<uintptr_t>(yp) |
                         reinterpret_cast<uintptr_t>(out.data_ptr())) & 15) == 0;
  if (!aligned) {                                   // a view at an odd offset: realign first
    x = x.clone();
    if (yp) {
      yc = yc.clone();
      yp = yc.data_ptr();
    }
  }
  rc_ok(nsdb_mix64(x.data_ptr(), yp, out.data_ptr(), x.numel(), stream()), "mix64");
  return out;
}

// Group-by of keys that arrive in runs (relops.hip run_*_kernel): (reps [g], aggs [g, F], counts [g], first [g]) with
// the groups in row order, or an empty list when the keys are not ordered (some key below its predecessor: equal
// keys may then be apart) and the caller must take hash_aggregate. vals as in hash_aggregate; one host read (the
// group count and the order flag together).
std::vector<torch::Tensor> run_aggregate(torch::Tensor keys, c10::optional<torch::Tensor> vals, const std::string& op) {
  TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64 && keys.dim() == 1, "keys must be 1-D int64 GPU");
  keys = keys.contiguous();
  const int64_t n = keys.numel();
  const int opc = op_code(op);
  const AggVals a = agg_vals(vals, keys, false);
  const int F = a.F;
  auto i64 = keys.options().dtype(torch::kInt64);
  if (n == 0) return {};
  const int64_t T = nsdb::compact_tiles(n);
  auto cnt = torch::empty({T}, keys.options().dtype(torch::kInt32));
  auto off = torch::empty({T + 2}, i64);
  rc_ok(nsdb_run_count(keys.data_ptr(), n, reinterpret_cast<unsigned*>(cnt.data_ptr<int32_t>()),
                       LL(off.data_ptr<int64_t>()), stream()), "run_count");
  const auto st = off.slice(0, T, T + 2).cpu();          // [groups, descending step seen]
  const int64_t G = st[0].item<int64_t>();
  if (st[1].item<int64_t>() != 0) return {};
  auto heads = torch::empty({G}, i64), okey = torch::empty({G}, i64), ocnt = torch::empty({G}, i64);
  auto oagg = torch::empty({G, F}, keys.options().dtype(a.dtype));
  rc_ok(nsdb_run_reduce(keys.data_ptr(), a.ptr(), a.vrs, a.vcs, F, a.vt, opc, n, LL(off.data_ptr<int64_t>()),
                        G, LL(heads.data_ptr<int64_t>()), LL(okey.data_ptr<int64_t>()), F ? oagg.data_ptr() : nullptr,
                        LL(ocnt.data_ptr<int64_t>()), stream()), "run_reduce");
  return {okey, oagg, ocnt, heads};
}


// Rows idx of several device columns in one launch (relops.hip take_many_kernel). Every column: a contiguous tensor
// on idx's device whose rows (dim 0) are 1, 2, 4, 8 or a multiple of 16 bytes wide (narrower multi-byte rows are
// copied element by element). Returns the gathered columns and a device flag word (1: an id was out of range).
// bad: an int32 device word the kernel sets on an out-of-range id (kept by the caller across calls and checked with
// its other reads: no per-call fill launch)
std::vector<torch::Tensor> take_many(std::vector<torch::Tensor> cols, torch::Tensor idx, torch::Tensor bad) {
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt64 && idx.dim() == 1, "take_many: idx 1-D int64 GPU");
  TORCH_CHECK(bad.is_cuda() && bad.device() == idx.device() && bad.scalar_type() == torch::kInt32 && bad.numel() >= 1,
              "take_many: bad must be an int32 word on idx's device");
  idx = idx.contiguous();
  const int64_t n = idx.numel();
  std::vector<torch::Tensor> out;
  out.reserve(cols.size());
  std::vector<const void*> src;
  std::vector<void*> dst;
  std::vector<long long> nsrc;
  std::vector<int> w, per;
  auto flush = [&]() {
    if (!src.empty())
      rc_ok(nsdb_take_many(src.data(), dst.data(), nsrc.data(), w.data(), per.data(), (int)src.size(),
                           LL(idx.data_ptr<int64_t>()), n, bad.data_ptr<int>(), stream()), "take_many");
    src.clear(); dst.clear(); nsrc.clear(); w.clear(); per.clear();
  };
  for (auto& c : cols) {
    TORCH_CHECK(c.is_cuda() && c.device() == idx.device() && c.dim() >= 1 && c.is_contiguous(),
                "take_many: contiguous columns on idx's device expected");
    auto sizes = c.sizes().vec();
    sizes[0] = n;
    auto o = torch::empty(sizes, c.options());
    out.push_back(o);
    TORCH_CHECK(n == 0 || c.size(0) > 0, "take_many: row ids into an empty column");
    const int64_t rowb = c.numel() == 0 ? 0 : (int64_t)c.nbytes() / c.size(0);
    if (n == 0 || rowb == 0) continue;
    int ww, pp;
    if (rowb == 1 || rowb == 2 || rowb == 4 || rowb == 8) { ww = (int)rowb; pp = 1; }
    else if (rowb % 16 == 0) { ww = 16; pp = (int)(rowb / 16); }
    else { ww = (int)c.element_size(); pp = (int)(rowb / ww); }
    if (reinterpret_cast<uintptr_t>(c.data_ptr()) % ww != 0) {   // a view at an offset: element-wide copies
      ww = (int)c.element_size();
      pp = (int)(rowb / ww);
    }
    src.push_back(c.data_ptr()); dst.push_back(o.data_ptr()); nsrc.push_back(c.size(0)); w.push_back(ww); per.push_back(pp);
    if ((int)src.size() == nsdb::kTakeCols) flush();
  }
  flush();
  return out;
}

// The key columns of an ORDER BY: 1..4 one-dimensional int32 / int64 / float32 / float64 GPU columns of equal length,
// made contiguous in place (keys keeps them alive); dt: dtype codes (sort_plan.h), ds: 1 = descending.
struct OrderKeys {
  int m = 0;
  int64_t n = 0;
  const void* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
  int dt[4] = {0, 0, 0, 0}, ds[4] = {0, 0, 0, 0};
};
OrderKeys order_keys(std::vector<torch::Tensor>& keys, const std::vector<bool>& desc, const char* who) {
  OrderKeys k;
  k.m = (int)keys.size();
  TORCH_CHECK(k.m >= 1 && k.m <= 4, who, ": 1 to 4 key columns");
  TORCH_CHECK((int)desc.size() == k.m, who, ": one direction per key");
  k.n = keys[0].numel();
  for (int j = 0; j < k.m; ++j) {
    auto& c = keys[j];
    TORCH_CHECK(c.is_cuda() && c.dim() == 1 && c.numel() == k.n && c.device() == keys[0].device(), who,
                ": keys must be 1-D GPU columns of equal length on one device");
    const auto t = c.scalar_type();
    k.dt[j] = t == torch::kInt32 ? 0 : t == torch::kFloat32 ? 1 : t == torch::kInt64 ? 2 : t == torch::kFloat64 ? 3 : -1;
    TORCH_CHECK(k.dt[j] >= 0, who, ": keys must be int32, int64, float32 or float64");
    c = c.contiguous();
    k.ptr[j] = c.data_ptr();
    k.ds[j] = desc[j] ? 1 : 0;
  }
  return k;
}

// ORDER BY keys[0], keys[1], ... LIMIT k (topk.hip): the int64 row ids of the min(k, n) first rows in final order;
// desc[j]: key j orders descending; equal rows by ascending row id. Keys: 1..4 one-dimensional int32 / int64 /
// float32 / float64 GPU columns of equal length n < 2^31 (read in place at their native width), min(k, n) <= 2048.
// No host read: a linear chain of launches on the current stream, scratch from the caching allocator.
torch::Tensor order_limit(std::vector<torch::Tensor> keys, std::vector<bool> desc, int64_t k) {
  const OrderKeys ok = order_keys(keys, desc, "order_limit");
  const int m = ok.m;
  const int64_t n = ok.n;
  auto i64 = keys[0].options().dtype(torch::kInt64);
  if (n == 0 || k <= 0) return torch::empty({0}, i64);
  TORCH_CHECK(n < (int64_t(1) << 31), "order_limit: at most 2^31 - 1 rows");
  const int64_t k_eff = std::min<int64_t>(k, n);
  TORCH_CHECK(k_eff <= nsdb_order_limit_max_k(), "order_limit: k above ", nsdb_order_limit_max_k());
  const int64_t sbytes = nsdb_order_limit_state_bytes(ok.dt, m, n);
  TORCH_CHECK(sbytes > 0, "order_limit: bad key set");
  auto i32 = keys[0].options().dtype(torch::kInt32);
  auto state = torch::zeros({(sbytes + 7) / 8}, i64);
  auto lists = torch::empty({2 * n}, i32);
  auto win = torch::empty({k_eff}, i32);
  auto out = torch::empty({k_eff}, i64);
  rc_ok(nsdb_order_limit(ok.ptr, ok.dt, ok.ds, m, n, k, state.data_ptr(), reinterpret_cast<unsigned*>(lists.data_ptr<int>()),
                         reinterpret_cast<unsigned*>(win.data_ptr<int>()), LL(out.data_ptr<int64_t>()), stream()),
        "order_limit");
  return out;
}

// The launch plan of order_by for these key dtype codes (0 int32, 1 float32, 2 int64, 3 float64) and n rows
// (sort_plan.h); launches nothing. rc: 0, -1 bad key count, -2 bad dtype, -3 n outside [1, 2^31).
pybind11::dict order_by_plan(std::vector<int64_t> dtypes, int64_t n) {
  int dt[4] = {0, 0, 0, 0};
  const int m = (int)dtypes.size();
  for (int j = 0; j < m && j < 4; ++j) dt[j] = (int)dtypes[j];
  long long f[12];
  nsdb_order_by_plan(dt, m, n, f);
  static const char* names[12] = {"rc", "word_bits", "tile", "tiles", "passes", "launches", "scan_step", "state_bytes",
                                  "counts_bytes", "words_bytes", "ids_bytes", "scratch_bytes"};
  pybind11::dict d;
  for (int i = 0; i < 12; ++i) d[names[i]] = (int64_t)f[i];
  return d;
}

// ORDER BY keys[0], keys[1], ... (sort.hip): the int64 row ids of all n rows in final order, or of the first `limit`
// (limit < 0: all). Keys and order as order_limit. No host read: a linear chain of launches on the current stream, every
// scratch buffer sized by the plan and taken from the caching allocator.
torch::Tensor order_by(std::vector<torch::Tensor> keys, std::vector<bool> desc, int64_t limit) {
  const OrderKeys ok = order_keys(keys, desc, "order_by");
  const int m = ok.m;
  const int64_t n = ok.n;
  auto i64 = keys[0].options().dtype(torch::kInt64);
  if (n == 0 || limit == 0) return torch::empty({0}, i64);
  TORCH_CHECK(n < (int64_t(1) << 31), "order_by: at most 2^31 - 1 rows");
  const int64_t lim = limit < 0 ? n : std::min<int64_t>(limit, n);
  long long f[12];
  TORCH_CHECK(nsdb_order_by_plan(ok.dt, m, n, f) == 0, "order_by: bad key set (plan code ", f[0], ")");
  const int64_t state_b = f[7], counts_b = f[8], words_b = f[9], ids_b = f[10];
  auto state = torch::zeros({(state_b + 7) / 8}, i64);
  auto counts = torch::empty({(counts_b + 7) / 8}, i64);
  auto words = torch::empty({(words_b + 7) / 8}, i64);
  auto ids = torch::empty({(ids_b + 7) / 8}, i64);
  auto out = torch::empty({lim}, i64);
  rc_ok(nsdb_order_by(ok.ptr, ok.dt, ok.ds, m, n, lim, state.data_ptr(), counts.data_ptr(), words.data_ptr(), ids.data_ptr(),
                      LL(out.data_ptr<int64_t>()), stream()),
        "order_by");
  return out;
}

// The plan of hash_aggregate for n rows and F value columns under the current MID setting (relops_plan.h agg_plan);
// launches nothing. scratch_low / scratch_part: status[4] of a call that ends on the LOW (or MID) / the PART path.
pybind11::dict hash_aggregate_plan(int64_t n, int64_t F, int64_t low_threshold, bool want_inv, bool want_first) {
  const nsdb::AggPlan p = nsdb::agg_plan(n, (int)F, low_threshold, g_agg_mid, want_inv, want_first);
  pybind11::dict d;
  d["rc"] = p.rc;
  if (p.rc != nsdb::AGG_OK) return d;
  const std::pair<const char*, int64_t> f[] = {
      {"lcap_low", p.lcap_low}, {"lcap_part", p.lcap_part}, {"lcap_mid", p.lcap_mid}, {"gcap_low", p.glow.cap},
      {"gcap_part", p.gpart.cap}, {"low_thr", p.low_thr}, {"pbits", p.pbits}, {"P", p.P}, {"G", p.G}, {"rpw", p.rpw},
      {"T", p.T}, {"T2", p.T2}, {"ocap_low", p.ocap_low}, {"table_words_low", p.glow.words},
      {"table_words_part", p.gpart.words}, {"work_bytes", p.work.total}, {"phase1_bytes", p.phase1_bytes},
      {"part_bytes", p.part_bytes}, {"scratch_low", p.phase1_bytes},
      {"scratch_part", p.phase1_bytes + p.part_bytes - 8 * nsdb::agg_out(p.ocap_low, p.F).words}};
  for (const auto& kv : f) d[kv.first] = kv.second;
  return d;
}

// The plan of join_build for n build rows under the current filter / partition settings (relops_plan.h join_plan);
// launches nothing. bloom_words and stat_words are the sizes of join_build's third and fourth tensors.
pybind11::dict join_build_plan(int64_t n) {
  const nsdb::JoinPlan p = join_plan_now(n, 0);
  pybind11::dict d;
  const std::pair<const char*, int64_t> f[] = {
      {"load", p.load}, {"cap", p.cap}, {"regions", p.regions}, {"part", p.part}, {"bloom_words", p.W},
      {"bshift", p.bshift}, {"fold", p.fold}, {"stat_words", p.regions ? 2 : 0}, {"rc", p.part ? p.work.rc : 0},
      {"P", p.work.P}, {"G", p.work.G}, {"Pc", p.work.Pc}, {"sh", p.work.sh}, {"rpw", p.work.rpw},
      {"work_bytes", p.work.total}};
  for (const auto& kv : f) d[kv.first] = kv.second;
  return d;
}
}  // namespace

std::vector<torch::Tensor> hash_aggregate_impl(torch::Tensor keys, c10::optional<torch::Tensor> vals,
                                               const std::string& op, bool want_inv, int64_t low_threshold) {
  return hash_aggregate(keys, vals, op, want_inv, low_threshold, true, pybind11::none());
}

void register_relops(pybind11::module& m) {
  m.def("hash_aggregate", &hash_aggregate,
        "device hash group-by + aggregate: (reps, aggs, counts, first, inv, status[g, path, ok, sample_distinct, scratch_bytes])",
        pybind11::arg("keys"), pybind11::arg("vals") = pybind11::none(), pybind11::arg("op") = "sum",
        pybind11::arg("want_inv") = false, pybind11::arg("low_threshold") = 0, pybind11::arg("want_first") = true,
        pybind11::arg("scratch") = pybind11::none());
  m.def("hash_aggregate_plan", &hash_aggregate_plan, "plan of hash_aggregate for n rows and F value columns: table "
        "capacities, PART geometry and the scratch bytes of either path; launches nothing", pybind11::arg("n"),
        pybind11::arg("F"), pybind11::arg("low_threshold") = 0, pybind11::arg("want_inv") = false,
        pybind11::arg("want_first") = true);
  m.def("join_build_plan", &join_build_plan, "plan of join_build for n build rows: load factor, slots, table kind, "
        "probe filter and partition geometry; launches nothing", pybind11::arg("n"));
  m.def("take_many", &take_many, "rows idx of several device columns in one launch (bad: int32 device word set on "
        "an out-of-range id)", pybind11::arg("cols"), pybind11::arg("idx"), pybind11::arg("bad"));
  m.def("join_build", &join_build, "device hash-join build: (table, perm, probe filter (empty: none), host [fail, "
        "largest extra-row count] (empty: not read))");
  m.def("join_probe", &join_probe, "device hash-join probe: (build_idx, probe_idx)", pybind11::arg("tab"),
        pybind11::arg("perm"), pybind11::arg("keys"), pybind11::arg("bloom") = pybind11::none());
  m.def("join_set_bloom", [](bool on, int64_t min_table_bytes, int64_t max_filter_bytes) {
          g_join_bloom = on;
          g_join_bloom_min_bytes = min_table_bytes;
          g_join_bloom_max_bytes = max_filter_bytes;
        }, "build probe filters for join tables of more than min_table_bytes of slots whose filter has at most "
        "max_filter_bytes (default on, 4 MiB, 4 MiB)",
        pybind11::arg("on"), pybind11::arg("min_table_bytes") = int64_t(4) << 20,
        pybind11::arg("max_filter_bytes") = int64_t(4) << 20);
  m.def("join_set_part", [](bool on) { g_join_part = on; }, "partitioned LDS-region build of join tables of more than "
        "one 4096-slot region (default on; off: the global-atomic insert)", pybind11::arg("on"));
  m.def("partition_perm", &partition_perm, "stable device partition permutation: (perm, counts)");
  m.def("agg_set_mid", [](bool on) { g_agg_mid = on; }, "enable / disable the MID group-by path (hash-partitioned LDS "
        "tables sharing their rows through L2); returns nothing", pybind11::arg("on"));
  m.def("compact", &compact, "row ids of the set rows of a 0/1 byte mask, in order (stable stream compaction)",
        pybind11::arg("mask"));
  m.def("run_aggregate", &run_aggregate, "group-by of keys arriving in runs: (reps, aggs, counts, first) or [] when "
        "the keys are not ordered", pybind11::arg("keys"), pybind11::arg("vals") = pybind11::none(),
        pybind11::arg("op") = "sum");
  m.def("order_limit", &order_limit, "ORDER BY keys (desc[j]: key j descending; ties by row id) LIMIT k: int64 row ids "
        "in final order, no host read", pybind11::arg("keys"), pybind11::arg("desc"), pybind11::arg("k"));
  m.attr("ORDER_LIMIT_MAX_K") = nsdb_order_limit_max_k();
  m.def("order_by", &order_by, "ORDER BY keys (desc[j]: key j descending; ties by row id): int64 row ids of all rows, "
        "or of the first `limit` (< 0: all), in final order, no host read", pybind11::arg("keys"), pybind11::arg("desc"),
        pybind11::arg("limit") = -1);
  m.def("order_by_plan", &order_by_plan, "launch plan of order_by for dtype codes (0 i32, 1 f32, 2 i64, 3 f64) and n "
        "rows: rc, word_bits, tile, tiles, passes, launches, scan_step and the scratch bytes by buffer",
        pybind11::arg("dtypes"), pybind11::arg("n"));
  m.attr("ORDER_BY_TILE") = nsdb_order_by_tile();
  m.def("mix64", &mix64, "key hash mix64((x ^ y) + GOLD) per row, one pass", pybind11::arg("x"),
        pybind11::arg("y") = pybind11::none());
}
