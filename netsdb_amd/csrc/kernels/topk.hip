// Device ORDER BY ... LIMIT k (execution/kernels.py order_limit): the row ids of the k first rows under a lexicographic
// order over 1..4 key columns (int32 / int64 / float32 / float64, each ascending or descending), ties broken by
// ascending row id. MSD radix select over 8-bit digits, then one workgroup sorts the <= 2048 winners in LDS.
//
// Order words. Every key element maps in registers to an unsigned order word (32 significant bits for 4-byte keys, 64
// for 8-byte ones) whose unsigned order is the contract's order: signed ints flip the sign bit; floats fold -0.0
// into +0.0, map every NaN to the top word (above +inf) and take the sign-magnitude flip; a descending key is
// complemented. Columns are read in their native width. The problem is then always "the k smallest of
// (w0, .., w_{m-1}, row id)", a total order, so the selection ends with exactly min(k, n) winners.
//
// Passes (launch count and grids depend only on n, the key widths and k; every kernel reads its extents from the
// device state and returns at once when nothing is left):
//   ol_diff_kernel   one pass over all key columns: per key the OR of (word ^ word of row 0), i.e. the bits in which
//                    the column varies at all. Digits are taken only below each key's highest varying bit (a key
//                    that is constant has no digit), so int64 columns holding small integers and floats of one
//                    binade cost no pass per shared leading digit.
//   ol_hist0_kernel  histogram of digit 0 over the column of the first varying key (LDS bins, one global integer
//                    atomic per non-empty bin per workgroup).
//   ol_pass_kernel p every workgroup finds the pivot bin of digit p (the bin holding the need-th row) from the 256
//                    bins, appends rows below it to the winners and rows inside it to the other candidate list
//                    (int32 row ids; one cursor atomic per list per 1024-row tile), and histograms digit p + 1 of
//                    those candidates in the same sweep. When the pivot bin holds exactly the rows still wanted they
//                    all win and the selection is over. Pass 0 sweeps the rows themselves, later passes only the
//                    candidate list (ping-pong between two n-entry lists).
//   ol_sort_kernel   one workgroup: bitonic sort of the winners by the full multi-word comparator in LDS
//                    (<= 2048 x (4 words + id + slot) = 80 KB), int64 ids out.
// Bound on FULL-COLUMN passes, whatever the data: one over every key column (diff), one over one key column (hist0)
// and one over at most two key columns (pass 0; the second only for rows of the pivot bin): 3. Every later pass
// walks a candidate list, which holds only the rows equal to the k-th row on all digits seen so far.
//
// Integer atomics only; the winners are a set fixed by the total order and the final sort orders them, so the output
// is bit-for-bit reproducible although list order is not. No host synchronisation: the launch chain is linear on one
// stream and capturable into a graph. The state (nsdb_order_limit_state_bytes) must be zeroed by the caller.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace nsdb_topk {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef long long i64;

constexpr int kMaxKeys = 4;
constexpr int kMaxK = 2048;
constexpr int kBins = 256;
constexpr int kThreads = 256;
constexpr int kGridCap = 2048;
constexpr int kUnroll = 4;            // rows per thread in flight in the sweeps
constexpr int kTile = kThreads * kUnroll;
// state layout in u32 words: diff[4] (u64) | nwin | need[p] | cnt[p] | hist[p][256]
constexpr int kNwinOff = 8, kNeedOff = 16, kCntOff = 64, kHistOff = 128, kPassCap = 44;

#include "order_words.h"   // DT_*, Keys, word_at, key_word

struct Spec {
  int key;      // key index, K.m for the row id, -1: there is no such digit
  int shift;
  u32 mask;
};

// Digit p of the concatenated digit string: the digits of each key below its highest varying bit, then the row id's.
__device__ __forceinline__ Spec spec_of(const u32* st, const Keys& K, int p) {
  const u64* diff = reinterpret_cast<const u64*>(st);
  Spec s{-1, 0, 0};
  int q = p;
  bool found = false;
#pragma unroll
  for (int j = 0; j <= kMaxKeys; ++j) {
    if (j <= K.m && !found) {
      int bits;
      if (j < K.m) {
        const u64 d = diff[j < kMaxKeys ? j : 0];
        bits = d ? 64 - __clzll((i64)d) : 0;
      } else {
        bits = K.idbits;
      }
      const int nd = (bits + 7) >> 3;
      if (q < nd) {
        const int hi = bits - 8 * q;
        const int w = hi < 8 ? hi : 8;
        s.key = j;
        s.shift = hi - w;
        s.mask = (1u << w) - 1u;
        found = true;
      } else {
        q -= nd;
      }
    }
  }
  return s;
}

// the word digit s is taken from: key s.key's order word of row id, or the row id itself
__device__ __forceinline__ u64 word_of(const Keys& K, int key, u32 id) {
  return key == K.m ? (u64)id : key_word(K, key, (i64)id);
}

__device__ __forceinline__ u32 digit_of(const Keys& K, const Spec& s, u32 id) {
  return (u32)(word_of(K, s.key, id) >> s.shift) & s.mask;
}

__device__ __forceinline__ void flush_bins(const u32* lh, u32* gh) {
  for (int b = threadIdx.x; b < kBins; b += blockDim.x) {
    const u32 c = lh[b];
    if (c) atomicAdd(&gh[b], c);
  }
}

// ------------------------------------------------------------------------------------------------ diff
__global__ __launch_bounds__(kThreads) void ol_diff_kernel(Keys K, i64 n, u32 k_eff, u32* __restrict__ st) {
  __shared__ u64 red[kMaxKeys][kThreads / 64];
  u64 acc[kMaxKeys], first[kMaxKeys];
#pragma unroll
  for (int j = 0; j < kMaxKeys; ++j) {
    acc[j] = 0;
    first[j] = j < K.m ? word_at(K.p[j], K.dt[j], K.desc[j], 0) : 0;
  }
  const i64 step = (i64)gridDim.x * kThreads * kUnroll;
  for (i64 base = (i64)blockIdx.x * kThreads * kUnroll; base < n; base += step) {
#pragma unroll
    for (int j = 0; j < kMaxKeys; ++j) {
      if (j < K.m) {
        u64 w[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const i64 i = base + u * kThreads + threadIdx.x;
          w[u] = i < n ? word_at(K.p[j], K.dt[j], K.desc[j], i) : first[j];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) acc[j] |= w[u] ^ first[j];
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kMaxKeys; ++j) {
    u64 v = acc[j];
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    if (lane == 0) red[j][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMaxKeys) {
    u64 v = 0;
    for (int w = 0; w < kThreads / 64; ++w) v |= red[threadIdx.x][w];
    if (v && (int)threadIdx.x < K.m) atomicOr(reinterpret_cast<u64*>(st) + threadIdx.x, v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) st[kNeedOff] = k_eff;
}

// ------------------------------------------------------------------------------------------------ hist 0
__global__ __launch_bounds__(kThreads) void ol_hist0_kernel(Keys K, i64 n, u32* __restrict__ st) {
  __shared__ u32 lh[kBins];
  for (int b = threadIdx.x; b < kBins; b += kThreads) lh[b] = 0;
  const Spec s = spec_of(st, K, 0);
  __syncthreads();
  const i64 step = (i64)gridDim.x * kThreads * kUnroll;
  for (i64 base = (i64)blockIdx.x * kThreads * kUnroll; base < n; base += step) {
    u32 d[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const i64 i = base + u * kThreads + threadIdx.x;
      d[u] = i < n ? digit_of(K, s, (u32)i) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
      if (d[u] < (u32)kBins) atomicAdd(&lh[d[u]], 1u);
  }
  __syncthreads();
  flush_bins(lh, st + kHistOff);
}

// ------------------------------------------------------------------------------------------------ pass p
__global__ __launch_bounds__(kThreads) void ol_pass_kernel(Keys K, i64 n, int p, u32 k_eff, u32* __restrict__ st,
                                                           const u32* __restrict__ lin, u32* __restrict__ lout,
                                                           u32* __restrict__ win) {
  __shared__ u32 lh[kBins];
  __shared__ u32 wsum[kThreads / 64];
  __shared__ u32 wtot[2][kThreads / 64];
  __shared__ u32 bases[2];
  __shared__ u32 piv[3];
  const u32 need = st[kNeedOff + p];
  if (need == 0) return;                                      // the selection is over
  const u32 cnt = p == 0 ? (u32)n : st[kCntOff + p];
  if (blockIdx.x != 0 && (u64)blockIdx.x * kTile >= cnt) return;
  const Spec s0 = spec_of(st, K, p);
  if (s0.key < 0) return;
  const Spec s1 = spec_of(st, K, p + 1);
  // pivot: the bin b with excl(b) < need <= incl(b)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 h = st[kHistOff + p * kBins + tid];
  u32 incl = h;
  for (int o = 1; o < 64; o <<= 1) {
    const u32 t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  lh[tid] = 0;
  if (tid == 0) {                                             // (bins that do not add up to need: nothing is a candidate)
    piv[0] = 0xFFFFFFFEu;
    piv[1] = need;
    piv[2] = 0;
  }
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += wsum[w];
  const u32 excl = incl - h;
  if (excl < need && need <= incl) {
    piv[0] = (u32)tid;
    piv[1] = excl;
    piv[2] = h;
  }
  __syncthreads();
  const u32 b = piv[0], rem = need - piv[1];
  const bool all_win = rem == piv[2];                         // the pivot bin holds exactly the rows still wanted
  if (blockIdx.x == 0 && tid == 0) st[kNeedOff + p + 1] = all_win ? 0u : rem;
  u32* nwin = st + kNwinOff;
  u32* ncand = st + kCntOff + p + 1;
  // Tiles of kTile rows: every thread classifies kUnroll rows, one block scan ranks the tile's winners and candidates
  // (counts packed winners << 16 | candidates), and ONE cursor atomic per list per tile reserves their places (a
  // pivot bin can hold nearly every row: doubles of one sign share most of digit 0).
  int it = 0;
  for (u64 base = (u64)blockIdx.x * kTile; base < cnt; base += (u64)gridDim.x * kTile, it ^= 1) {
    u32 id[kUnroll];
    u64 w[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const u64 i = base + u * kThreads + tid;
      id[u] = i < cnt ? (p == 0 ? (u32)i : lin[i]) : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) w[u] = id[u] != 0xFFFFFFFFu ? word_of(K, s0.key, id[u]) : 0;
    u32 cmask = 0, wmask = 0;
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const u32 d = id[u] != 0xFFFFFFFFu ? ((u32)(w[u] >> s0.shift) & s0.mask) : 0xFFFFFFFFu;
      if (d < b || (all_win && d == b)) wmask |= 1u << u;
      if (!all_win && d == b) cmask |= 1u << u;
    }
    const u32 mine = ((u32)__popc(wmask) << 16) | (u32)__popc(cmask);
    u32 inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
      const u32 t = __shfl_up(inc, o);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[it][wave] = inc;
    __syncthreads();
    u32 before = 0, total = 0;
    for (int x = 0; x < kThreads / 64; ++x) {
      const u32 t = wtot[it][x];
      if (x < wave) before += t;
      total += t;
    }
    if (total == 0) continue;                                 // (block-uniform)
    if (tid == 0) {
      if (total & 0xFFFFu) bases[0] = atomicAdd(ncand, total & 0xFFFFu);
      if (total >> 16) bases[1] = atomicAdd(nwin, total >> 16);
    }
    __syncthreads();
    const u32 excl_me = before + inc - mine;
    u32 cpos = bases[0] + (excl_me & 0xFFFFu), wpos = bases[1] + (excl_me >> 16);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (wmask & (1u << u)) {
        if (wpos < k_eff) win[wpos] = id[u];
        ++wpos;
      }
      if (cmask & (1u << u)) {
        if (cpos < (u32)n) lout[cpos] = id[u];
        ++cpos;
        if (s1.key >= 0) {
          const u64 w1 = s1.key == s0.key ? w[u] : word_of(K, s1.key, id[u]);
          atomicAdd(&lh[(u32)(w1 >> s1.shift) & s1.mask], 1u);
        }
      }
    }
  }
  __syncthreads();
  if (!all_win && s1.key >= 0) flush_bins(lh, st + kHistOff + (p + 1) * kBins);
}

// ------------------------------------------------------------------------------------------------ final sort
__global__ __launch_bounds__(1024) void ol_sort_kernel(Keys K, u32 n, u32 W, u32 P2,
                                                       const u32* __restrict__ win, i64* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  u64* words = reinterpret_cast<u64*>(lds_raw);                // [m][P2]
  u32* ids = reinterpret_cast<u32*>(words + (size_t)K.m * P2);  // [P2]
  u32* perm = ids + P2;                                        // [P2]
  for (u32 t = threadIdx.x; t < P2; t += blockDim.x) {
    perm[t] = t;
    if (t < W) {
      u32 id = win[t];
      if (id >= n) id = n - 1;                                 // (never: the selection ends with exactly W winners)
      ids[t] = id;
#pragma unroll
      for (int j = 0; j < kMaxKeys; ++j)
        if (j < K.m) words[(size_t)j * P2 + t] = word_at(K.p[j], K.dt[j], K.desc[j], (i64)id);
    }
  }
  __syncthreads();
  auto less = [&](u32 a, u32 c) -> bool {   // slots >= W are padding: above every row
    if (a >= W) return false;
    if (c >= W) return true;
    for (int j = 0; j < K.m; ++j) {
      const u64 wa = words[(size_t)j * P2 + a], wc = words[(size_t)j * P2 + c];
      if (wa != wc) return wa < wc;
    }
    return ids[a] < ids[c];
  };
  for (u32 size = 2; size <= P2; size <<= 1) {
    for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
      for (u32 t = threadIdx.x; t < P2 / 2; t += blockDim.x) {
        const u32 lo = 2 * t - (t & (stride - 1));
        const u32 hi = lo + stride;
        const bool up = (lo & size) == 0;
        const u32 a = perm[lo], c = perm[hi];
        if (up ? less(c, a) : less(a, c)) {
          perm[lo] = c;
          perm[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (u32 t = threadIdx.x; t < W; t += blockDim.x) out[t] = (i64)ids[perm[t]];
}

int key_bytes(int dt) { return dt == DT_I32 || dt == DT_F32 ? 4 : 8; }

int idbits_of(long long n) {
  int b = 1;
  while (b < 31 && (1ll << b) < n) ++b;
  return b;
}

// the largest number of digits the keys and the row id can have: the number of pass launches
int max_passes(const int* dt, int m, long long n) {
  int p = (idbits_of(n) + 7) / 8;
  for (int j = 0; j < m; ++j) p += key_bytes(dt[j]);
  return p;
}

}  // namespace nsdb_topk

extern "C" {

int nsdb_order_limit_max_k() { return nsdb_topk::kMaxK; }

// bytes of the (zeroed) device state for these key dtypes (0 int32, 1 float32, 2 int64, 3 float64) and n rows
long long nsdb_order_limit_state_bytes(const int* dt, int m, long long n) {
  using namespace nsdb_topk;
  if (m < 1 || m > kMaxKeys) return -1;
  return 4ll * (kHistOff + (long long)(max_passes(dt, m, n) + 1) * kBins);
}

// keys: m device columns of n rows; state: zeroed, nsdb_order_limit_state_bytes; lists: 2 n u32; win: min(k, n) u32;
// out: min(k, n) int64 row ids in final order.
int nsdb_order_limit(const void* const* keys, const int* dt, const int* desc, int m, long long n, long long k,
                     void* state, unsigned* lists, unsigned* win, long long* out, hipStream_t st) {
  using namespace nsdb_topk;
  if (m < 1 || m > kMaxKeys || n <= 0 || n >= (1ll << 31) || k <= 0) return (int)hipErrorInvalidValue;
  const long long k_eff = std::min(k, n);
  if (k_eff > kMaxK) return (int)hipErrorInvalidValue;
  Keys K{};
  for (int j = 0; j < m; ++j) {
    if (dt[j] < 0 || dt[j] > 3 || keys[j] == nullptr) return (int)hipErrorInvalidValue;
    K.p[j] = keys[j];
    K.dt[j] = dt[j];
    K.desc[j] = desc[j] ? 1 : 0;
  }
  K.m = m;
  K.idbits = idbits_of(n);
  const int P = max_passes(dt, m, n);
  if (P + 1 > kPassCap) return (int)hipErrorInvalidValue;
  u32* s32 = reinterpret_cast<u32*>(state);
  const unsigned gu = (unsigned)std::min<long long>(kGridCap, (n + kThreads * kUnroll - 1) / (kThreads * kUnroll));
  hipLaunchKernelGGL(ol_diff_kernel, dim3(gu), dim3(kThreads), 0, st, K, (i64)n, (u32)k_eff, s32);
  hipLaunchKernelGGL(ol_hist0_kernel, dim3(gu), dim3(kThreads), 0, st, K, (i64)n, s32);
  for (int p = 0; p < P; ++p) {
    const u32* lin = lists + (size_t)(p & 1) * n;
    u32* lout = lists + (size_t)((p + 1) & 1) * n;
    hipLaunchKernelGGL(ol_pass_kernel, dim3(gu), dim3(kThreads), 0, st, K, (i64)n, p, (u32)k_eff, s32, lin, lout, win);
  }
  u32 P2 = 1;
  while (P2 < (u32)k_eff) P2 <<= 1;
  const size_t lds = (size_t)P2 * (8 * m + 8);
  hipLaunchKernelGGL(ol_sort_kernel, dim3(1), dim3(1024), lds, st, K, (u32)n, (u32)k_eff, P2, (const u32*)win,
                     (i64*)out);
  return (int)hipGetLastError();
}
}
