// Device ORDER BY without LIMIT (execution/kernels.py order_by): the int64 row ids of all n rows (or of the first
// `limit`) under the lexicographic order over 1..4 key columns that topk.hip selects from, ties by ascending row id.
// Stable LSD radix sort over 8-bit digits of the order words (order_words.h), last key first; the initial order is the
// identity, so stability alone gives the row-id tie-break.
//
// Launch chain (sort_plan.h fixes the launch count, grids and scratch from the dtypes and n alone; every kernel of a
// dead pass reads its flag from the device state and returns at once):
//   os_hist_kernel     one pass over every key column in native width: all digit histograms of all keys in LDS
//                      (32 slots x 256 bins), non-empty bins flushed with integer atomics to the zeroed state.
//   os_plan_kernel     one workgroup: per slot `live` (no bin holds all n rows), the 256 exclusive bin bases and the
//                      number of live passes before it (its low bit is the source buffer); per key a live flag (a
//                      constant key is neither gathered nor passed over); per live pass whether a later pass of the
//                      same key reads the words it would write.
//   per key, last to first:
//     os_load_kernel   the key's order words gathered through the current ids (before any live pass the ids are the
//                      identity and are not read)
//     per byte, low to high:
//       os_count_kernel    per-tile digit counts, bin-major [256][T]
//       os_scan_kernel     one workgroup per bin: exclusive scan over the tiles, plus the bin base
//       os_scatter_kernel  stable rank inside the tile, (word, id) moved to the other buffer
//   os_out_kernel      int64 ids of the first `limit` rows from the buffer of the final parity.
//
// Rank inside a tile (os_scatter_kernel): wave w owns the w-th quarter of the tile and walks it in row order, 64 rows
// a step. A step ranks its lanes per digit with eight ballots (the lanes that agree with mine on every digit bit, in
// lane order) on top of the wave's running per-digit count in LDS, which the highest lane of each digit then advances.
// After the walk those counts are the wave totals; bin d's thread prefix-sums them over the waves and a block scan over
// the bins gives every row its place in the tile's digit order. Row order inside the tile is (wave, step, lane) =
// input order, so the sort is stable. The tile is staged in that order in LDS (48 KB of words and ids at 64-bit words)
// and stored from there: neighbouring lanes write neighbouring places of a bin, at the scanned tile base.
//
// No workgroup waits for another: phases are ordered by kernel boundaries only. Integer atomics only (LDS bins and
// the histogram flush), and every output position is a pure function of the input, so the result is bit-for-bit
// reproducible. Every scattered store is guarded by pos < n: whatever the state holds, nothing is written out of
// range. No host read, linear on one stream, capturable into a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sort_plan.h"

namespace nsdb_sort {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef long long i64;

constexpr int kMaxKeys = nsdb::kSortMaxKeys;

#include "order_words.h"   // DT_*, Keys, word_at, key_word

using namespace nsdb;

constexpr int kWaves = kSortThreads / 64;

// Add one to bin d of an LDS histogram for every lane with `valid`; a digit the whole wave shares (the leading bytes
// of small integers, of dates, of floats of one binade) costs one add instead of a 64-way conflict.
__device__ __forceinline__ void bin_add(u32* h, u32 d, bool valid) {
  const u64 act = __ballot(valid);
  if (act == 0) return;
  const int first = __ffsll((i64)act) - 1;
  const u32 d0 = (u32)__shfl((int)d, first, 64);
  const u64 same = __ballot(valid && d == d0);
  if (same == act) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[d0], (u32)__popcll(act));
  } else if (valid) {
    atomicAdd(&h[d], 1u);
  }
}

// ------------------------------------------------------------------------------------------------ histograms
__global__ __launch_bounds__(kSortThreads) void os_hist_kernel(Keys K, i64 n, u32* __restrict__ st) {
  __shared__ u32 lh[kSortSlots * kSortBins];
  for (int b = threadIdx.x; b < kSortSlots * kSortBins; b += kSortThreads) lh[b] = 0;
  __syncthreads();
  const i64 step = (i64)gridDim.x * kSortHistRows;
  for (i64 base = (i64)blockIdx.x * kSortHistRows; base < n; base += step) {
#pragma unroll
    for (int j = 0; j < kMaxKeys; ++j) {
      if (j < K.m) {
        const bool wide = K.dt[j] == DT_I64 || K.dt[j] == DT_F64;
#pragma unroll
        for (int u = 0; u < kSortHistRows / kSortThreads; ++u) {
          const i64 i = base + u * kSortThreads + threadIdx.x;
          const bool valid = i < n;
          const u64 w = valid ? word_at(K.p[j], K.dt[j], K.desc[j], i) : 0;
#pragma unroll
          for (int b = 0; b < 8; ++b)
            if (b < 4 || wide) bin_add(lh + (j * 8 + b) * kSortBins, (u32)(w >> (8 * b)) & 0xFFu, valid);
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSortSlots * kSortBins; b += kSortThreads) {
    const u32 c = lh[b];
    if (c) atomicAdd(&st[kSortHistOff + b], c);
  }
}

// ------------------------------------------------------------------------------------------------ plan
__global__ __launch_bounds__(kSortThreads) void os_plan_kernel(Keys K, i64 n, u32* __restrict__ st) {
  __shared__ u32 wsum[kWaves];
  __shared__ u32 wmax[kWaves];
  __shared__ u32 live[kSortSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int s = 0; s < kSortSlots; ++s) {
    const u32 h = st[kSortHistOff + s * kSortBins + tid];
    u32 incl = h, mx = h;
    for (int o = 1; o < 64; o <<= 1) {
      const u32 t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (u32)__shfl_xor((int)mx, o));
    if (lane == 63) wsum[wave] = incl;
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    u32 before = 0, m = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) before += wsum[w];
      m = max(m, wmax[w]);
    }
    st[kSortBaseOff + s * kSortBins + tid] = before + incl - h;
    // a slot no key uses has an empty histogram; one whose digit every row shares has a bin of n: both are dead
    if (tid == 0) live[s] = (m != 0 && m != (u32)n) ? 1u : 0u;
    __syncthreads();
  }
  if (tid == 0) {
    u32 done = 0;                                  // live passes so far, in execution order
    for (int j = kMaxKeys - 1; j >= 0; --j) {
      if (j >= K.m) continue;
      int last = -1;
      for (int b = 0; b < 8; ++b) {
        const int s = j * 8 + b;
        st[kSortLiveOff + s] = live[s];
        st[kSortBeforeOff + s] = done;
        st[kSortWriteOff + s] = 1;
        if (live[s]) {
          ++done;
          last = s;
        }
      }
      if (last >= 0) st[kSortWriteOff + last] = 0;   // the next key reloads its words (or the sort is over)
      st[kSortKeyLiveOff + j] = last >= 0 ? 1u : 0u;
    }
    st[kSortTotalOff] = done;
  }
}

// ------------------------------------------------------------------------------------------------ load
// words[parity][i] = key j's order word of the row at place i of the current order
template <typename W>
__global__ __launch_bounds__(kSortThreads) void os_load_kernel(Keys K, i64 n, int j, const u32* __restrict__ st,
                                                               W* __restrict__ words, const u32* __restrict__ ids) {
  if (!st[kSortKeyLiveOff + j]) return;
  const u32 before = st[kSortBeforeOff + j * 8];
  W* dst = words + (size_t)(before & 1u) * n;
  const u32* src = ids + (size_t)(before & 1u) * n;
  const i64 i = (i64)blockIdx.x * kSortThreads + threadIdx.x;
  if (i >= n) return;
  i64 id = i;
  if (before != 0) {
    id = (i64)src[i];
    if (id >= n) id = n - 1;                                   // (never: the ids are a permutation)
  }
  dst[i] = (W)key_word(K, j, id);
}

// ------------------------------------------------------------------------------------------------ count
template <typename W>
__global__ __launch_bounds__(kSortThreads) void os_count_kernel(i64 n, i64 T, int slot, int shift,
                                                                const u32* __restrict__ st,
                                                                const W* __restrict__ words,
                                                                u32* __restrict__ counts) {
  if (!st[kSortLiveOff + slot]) return;
  __shared__ u32 lh[kSortBins];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const W* src = words + (size_t)(st[kSortBeforeOff + slot] & 1u) * n;
  const i64 t0 = (i64)blockIdx.x * kSortTile;
#pragma unroll
  for (int u = 0; u < kSortRowsPerThread; ++u) {
    const i64 i = t0 + u * kSortThreads + threadIdx.x;
    const bool valid = i < n;
    const W w = valid ? src[i] : (W)0;
    bin_add(lh, (u32)(w >> shift) & 0xFFu, valid);
  }
  __syncthreads();
  counts[(size_t)threadIdx.x * T + blockIdx.x] = lh[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ scan
// workgroup d: counts[d][t] <- base[d] + sum of counts[d][0 .. t), kSortScanStep tiles a step
__global__ __launch_bounds__(kSortThreads) void os_scan_kernel(i64 T, int slot, const u32* __restrict__ st,
                                                               u32* __restrict__ counts) {
  if (!st[kSortLiveOff + slot]) return;
  __shared__ u32 wsum[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u32* row = counts + (size_t)blockIdx.x * T;
  u32 carry = st[kSortBaseOff + slot * kSortBins + blockIdx.x];
  int it = 0;
  for (i64 t0 = 0; t0 < T; t0 += kSortScanStep, it ^= 1) {
    const i64 t = t0 + tid;
    const u32 c = t < T ? row[t] : 0u;
    u32 incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const u32 x = __shfl_up(incl, o);
      if (lane >= o) incl += x;
    }
    if (lane == 63) wsum[it][wave] = incl;
    __syncthreads();
    u32 before = 0, total = 0;
    for (int w = 0; w < kWaves; ++w) {
      const u32 x = wsum[it][w];
      if (w < wave) before += x;
      total += x;
    }
    if (t < T) row[t] = carry + before + incl - c;
    carry += total;
  }
}

// ------------------------------------------------------------------------------------------------ scatter
template <typename W>
__global__ __launch_bounds__(kSortThreads) void os_scatter_kernel(i64 n, i64 T, int slot, int shift,
                                                                  const u32* __restrict__ st, W* __restrict__ words,
                                                                  u32* __restrict__ ids,
                                                                  const u32* __restrict__ counts) {
  if (!st[kSortLiveOff + slot]) return;
  __shared__ W sword[kSortTile];
  __shared__ u32 sid[kSortTile];
  __shared__ u32 delta[kSortBins];
  __shared__ u32 wsum[kWaves];
  __shared__ u32 wcnt_lds[kWaves * kSortBins];
  volatile u32* wcnt = wcnt_lds;                   // lanes of one wave read what another lane of it wrote a step ago
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32 before = st[kSortBeforeOff + slot];
  const bool write_words = st[kSortWriteOff + slot] != 0;
  const size_t so = (size_t)(before & 1u) * n, dso = (size_t)((before + 1) & 1u) * n;
  const W* wsrc = words + so;
  const u32* isrc = ids + so;
  W* wdst = words + dso;
  u32* idst = ids + dso;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) wcnt[w * kSortBins + tid] = 0;
  __syncthreads();
  // this wave's rows: kSortRowsPerThread steps of 64 consecutive rows
  const i64 r0 = (i64)blockIdx.x * kSortTile + (i64)wave * (64 * kSortRowsPerThread) + lane;
  const u64 below = (1ull << lane) - 1ull;
  W word[kSortRowsPerThread];
  u32 id[kSortRowsPerThread], rank[kSortRowsPerThread];
#pragma unroll
  for (int u = 0; u < kSortRowsPerThread; ++u) {
    const i64 i = r0 + u * 64;
    const bool valid = i < n;
    word[u] = valid ? wsrc[i] : (W)0;
    id[u] = valid ? (before != 0 ? isrc[i] : (u32)i) : 0u;
  }
#pragma unroll
  for (int u = 0; u < kSortRowsPerThread; ++u) {
    const bool valid = r0 + u * 64 < n;
    const u32 d = (u32)(word[u] >> shift) & 0xFFu;
    u64 peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const u64 v = __ballot(bit);
      peers &= bit ? v : ~v;
    }
    u32 r = 0;
    if (valid) {
      r = wcnt[wave * kSortBins + d] + (u32)__popcll(peers & below);
      if ((peers >> lane) == 1ull) wcnt[wave * kSortBins + d] = r + 1;   // the digit's highest lane advances the count
    }
    rank[u] = r;
  }
  __syncthreads();
  // bin tid: its rows' start inside the tile (block scan over the bins), each wave's start inside the bin, and the
  // distance from a tile place to the global place of the bin's rows
  {
    u32 c[kWaves], tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      c[w] = wcnt[w * kSortBins + tid];
      tot += c[w];
    }
    u32 incl = tot;
    for (int o = 1; o < 64; o <<= 1) {
      const u32 x = __shfl_up(incl, o);
      if (lane >= o) incl += x;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    u32 pos = incl - tot;
    for (int w = 0; w < wave; ++w) pos += wsum[w];
    delta[tid] = counts[(size_t)tid * T + blockIdx.x] - pos;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      wcnt[w * kSortBins + tid] = pos;
      pos += c[w];
    }
  }
  __syncthreads();
  // stage the tile in digit order in LDS, so that neighbouring lanes then store to neighbouring places of a bin
#pragma unroll
  for (int u = 0; u < kSortRowsPerThread; ++u) {
    if (r0 + u * 64 < n) {
      const u32 d = (u32)(word[u] >> shift) & 0xFFu;
      const u32 l = wcnt[wave * kSortBins + d] + rank[u];
      if (l < (u32)kSortTile) {
        sword[l] = word[u];
        sid[l] = id[u];
      }
    }
  }
  __syncthreads();
  const i64 t0 = (i64)blockIdx.x * kSortTile;
  const u32 rows = (u32)(n - t0 < (i64)kSortTile ? n - t0 : (i64)kSortTile);
#pragma unroll
  for (int u = 0; u < kSortRowsPerThread; ++u) {
    const u32 l = (u32)(u * kSortThreads + tid);
    if (l < rows) {
      const W w = sword[l];
      const u32 pos = delta[(u32)(w >> shift) & 0xFFu] + l;
      if (pos < (u32)n) {
        idst[pos] = sid[l];
        if (write_words) wdst[pos] = w;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ out
__global__ __launch_bounds__(kSortThreads) void os_out_kernel(i64 n, i64 limit, const u32* __restrict__ st,
                                                              const u32* __restrict__ ids, i64* __restrict__ out) {
  const i64 i = (i64)blockIdx.x * kSortThreads + threadIdx.x;
  if (i >= limit) return;
  const u32 total = st[kSortTotalOff];
  out[i] = total == 0 ? i : (i64)ids[(size_t)(total & 1u) * n + i];
}

template <typename W>
void launch_chain(const Keys& K, const int* dt, const SortPlan& p, i64 n, i64 limit, u32* st, void* words_v, u32* ids,
                  u32* counts, i64* out, hipStream_t s) {
  W* words = reinterpret_cast<W*>(words_v);
  const dim3 blk(kSortThreads);
  const unsigned rows_grid = (unsigned)((n + kSortThreads - 1) / kSortThreads);
  const unsigned T = (unsigned)p.tiles;
  hipLaunchKernelGGL(os_hist_kernel, dim3(p.hist_grid), blk, 0, s, K, n, st);
  hipLaunchKernelGGL(os_plan_kernel, dim3(1), blk, 0, s, K, n, st);
  for (int j = K.m - 1; j >= 0; --j) {
    hipLaunchKernelGGL(os_load_kernel<W>, dim3(rows_grid), blk, 0, s, K, n, j, (const u32*)st, words, (const u32*)ids);
    for (int b = 0; b < sort_key_bytes(dt[j]); ++b) {
      const int slot = j * 8 + b;
      hipLaunchKernelGGL(os_count_kernel<W>, dim3(T), blk, 0, s, n, (i64)T, slot, 8 * b, (const u32*)st,
                         (const W*)words, counts);
      hipLaunchKernelGGL(os_scan_kernel, dim3(kSortBins), blk, 0, s, (i64)T, slot, (const u32*)st, counts);
      hipLaunchKernelGGL(os_scatter_kernel<W>, dim3(T), blk, 0, s, n, (i64)T, slot, 8 * b, (const u32*)st, words, ids,
                         (const u32*)counts);
    }
  }
  hipLaunchKernelGGL(os_out_kernel, dim3((unsigned)((limit + kSortThreads - 1) / kSortThreads)), blk, 0, s, n, limit,
                     (const u32*)st, (const u32*)ids, out);
}

}  // namespace nsdb_sort

extern "C" {

int nsdb_order_by_tile() { return nsdb::kSortTile; }

// The plan of a call as 12 numbers: rc, word_bits, tile, tiles, passes, launches, scan_step, state_bytes,
// counts_bytes, words_bytes, ids_bytes, scratch_bytes. Returns rc.
int nsdb_order_by_plan(const int* dt, int m, long long n, long long* f) {
  const nsdb::SortPlan p = nsdb::sort_plan(dt, m, n);
  f[0] = p.rc; f[1] = p.word_bits; f[2] = p.tile; f[3] = p.tiles; f[4] = p.passes; f[5] = p.launches;
  f[6] = p.scan_step; f[7] = p.state_bytes; f[8] = p.counts_bytes; f[9] = p.words_bytes; f[10] = p.ids_bytes;
  f[11] = p.scratch_bytes;
  return p.rc;
}

// keys: m device columns of n rows; state: zeroed, plan.state_bytes; counts / words / ids: plan.*_bytes;
// out: limit (1 <= limit <= n) int64 row ids in final order.
int nsdb_order_by(const void* const* keys, const int* dt, const int* desc, int m, long long n, long long limit,
                  void* state, void* counts, void* words, void* ids, long long* out, hipStream_t st) {
  using namespace nsdb_sort;
  const nsdb::SortPlan p = nsdb::sort_plan(dt, m, n);
  if (p.rc != nsdb::SORT_OK || limit < 1 || limit > n) return (int)hipErrorInvalidValue;
  Keys K{};
  for (int j = 0; j < m; ++j) {
    if (keys[j] == nullptr) return (int)hipErrorInvalidValue;
    K.p[j] = keys[j];
    K.dt[j] = dt[j];
    K.desc[j] = desc[j] ? 1 : 0;
  }
  K.m = m;
  K.idbits = 0;
  if (p.word_bits == 32)
    launch_chain<u32>(K, dt, p, (i64)n, (i64)limit, (u32*)state, words, (u32*)ids, (u32*)counts, (i64*)out, st);
  else
    launch_chain<u64>(K, dt, p, (i64)n, (i64)limit, (u32*)state, words, (u32*)ids, (u32*)counts, (i64*)out, st);
  return (int)hipGetLastError();
}
}
