// Delimited-text parser for gfx950 (MI355X): a buffer of whole lines -> one typed column per field, for any flat schema.
//
// Four launches (textparse_plan.h), ordered by kernel boundaries only:
//   tp_count_kernel   one workgroup per 16 KiB tile: newlines in the tile (16-byte loads, a SWAR byte compare)
//   tp_scan_kernel    one workgroup: exclusive scan of the tile counts, kTextScanStep tiles a step with a carry; writes
//                     the row count (newlines, plus one for a last line without its newline) and resets the status words
//   tp_rows_kernel    one workgroup per tile: the row starts in file order. A lane holds the 16-bit newline mask of its
//                     16 bytes; its rank in the wave is a prefix sum of the lanes' counts (0..16, five bits) taken from
//                     five 64-bit ballots, the waves' totals go through LDS, the tile base is the scanned count
//   tp_decode_kernel  one lane per row, every field of the row in one walk. The field loop is wave-uniform, so the
//                     field's kind and output pointer are scalar loads from the kernel argument; inside a field each
//                     lane consumes its own bytes from a 16-byte register window refilled by aligned 16-byte loads.
//
// Every read is guarded twice over: a 16-byte load is issued only when it ends inside the ALLOCATION (alloc), otherwise
// the bytes up to the PAYLOAD end (n) are read one by one, and the decode never asks for a byte at or past the end of its
// row. Offsets are 32-bit (the plan refuses 2^31 bytes). Malformed text is reported, never chased: the lowest bad row and
// its code go through one 64-bit atomic min; cells outside the fast grammar are counted (and listed when a list is given)
// and left to the host. Integer atomics only; outputs are pure functions of the input.
//
// Built without fast-math: a float is (double)mantissa / 10^frac, one IEEE division of two exact doubles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "textparse_plan.h"

#ifdef __FAST_MATH__
#error "textparse.hip needs IEEE division: build without fast-math"
#endif

namespace nsdb_text {

using namespace nsdb;

typedef unsigned long long u64;
typedef unsigned int u32;
typedef long long i64;
typedef unsigned char u8;

constexpr int kWaves = kTextThreads / 64;
constexpr int kStep = kTextThreads * kTextLoad;      // bytes one workgroup takes per step

struct TextFields {
  void* out[kTextMaxFields];
  u8 kind[kTextMaxFields];
};

struct W16 {
  u64 lo, hi;
};

// bytes [a, a + 16) of the buffer (a a multiple of 16, a < n); bytes at or past n may hold anything
__device__ __forceinline__ W16 load16(const u8* __restrict__ buf, u32 a, u32 n, u32 alloc) {
  W16 w;
  if (a + 16u <= alloc) {                                    // a + 16 <= 2^31 + 15: no wrap
    const uint4 v = *reinterpret_cast<const uint4*>(buf + a);
    w.lo = ((u64)v.y << 32) | v.x;
    w.hi = ((u64)v.w << 32) | v.z;
  } else {
    w.lo = w.hi = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (a + k < n) w.lo |= (u64)buf[a + k] << (8 * k);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (a + 8 + k < n) w.hi |= (u64)buf[a + 8 + k] << (8 * k);
  }
  return w;
}

// bit i set where byte i of w equals c (exact: no borrow between bytes)
__device__ __forceinline__ u32 eq_mask8(u64 w, u64 c8) {
  const u64 x = w ^ c8, lo7 = 0x7F7F7F7F7F7F7F7Full;
  const u64 z = ~(((x & lo7) + lo7) | x | lo7);              // 0x80 where the byte of x is zero
  return (u32)(((z >> 7) * 0x0102040810204080ull) >> 56);
}

// the newline mask of the 16 bytes at i, bytes at or past n masked off
__device__ __forceinline__ u32 newline_mask(const u8* __restrict__ buf, u32 i, u32 n, u32 alloc) {
  if (i >= n) return 0;
  const W16 w = load16(buf, i, n, alloc);
  const u64 nl = 0x0A0A0A0A0A0A0A0Aull;
  const u32 m = eq_mask8(w.lo, nl) | (eq_mask8(w.hi, nl) << 8);
  const u32 valid = n - i;
  return valid >= 16 ? m : m & ((1u << valid) - 1u);
}

// ------------------------------------------------------------------------------------------------ count
__global__ __launch_bounds__(kTextThreads) void tp_count_kernel(const u8* __restrict__ buf, u32 n, u32 alloc,
                                                                u32* __restrict__ counts) {
  const u32 t0 = blockIdx.x * (u32)kTextTile;
  u32 c = 0;
#pragma unroll
  for (int it = 0; it < kTextLoadsPerThread; ++it)
    c += __builtin_popcount(newline_mask(buf, t0 + it * kStep + threadIdx.x * kTextLoad, n, alloc));
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  __shared__ u32 ws[kWaves];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 s = 0;
    for (int w = 0; w < kWaves; ++w) s += ws[w];
    counts[blockIdx.x] = s;
  }
}

// ------------------------------------------------------------------------------------------------ scan
// counts[t] <- sum of counts[0 .. t); state: rows | no bad row | no flagged cell
__global__ __launch_bounds__(kTextThreads) void tp_scan_kernel(const u8* __restrict__ buf, u32 n, u32 T,
                                                               u32* __restrict__ counts, u64* __restrict__ state) {
  __shared__ u32 wsum[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u32 carry = 0;
  int it = 0;
  for (u32 t0 = 0; t0 < T; t0 += kTextScanStep, it ^= 1) {
    const u32 t = t0 + tid;
    const u32 c = t < T ? counts[t] : 0u;
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
    if (t < T) counts[t] = carry + before + incl - c;
    carry += total;
  }
  if (tid == 0) {
    state[0] = (u64)carry + (buf[n - 1] != '\n' ? 1u : 0u);   // the last line may lack its newline
    state[1] = ~0ull;
    state[2] = 0;
    state[3] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ row starts
// starts[0] = 0, starts[k + 1] = 1 + the position of the k-th newline; a last line without a newline ends at a virtual
// one at n (starts[rows] = n + 1). Row r is [starts[r], starts[r + 1] - 1).
__global__ __launch_bounds__(kTextThreads) void tp_rows_kernel(const u8* __restrict__ buf, u32 n, u32 alloc,
                                                               const u32* __restrict__ counts, u32 rows,
                                                               u32* __restrict__ starts) {
  __shared__ u32 wc[2][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u64 lt = (1ull << lane) - 1;
  const u32 t0 = blockIdx.x * (u32)kTextTile;
  u32 base = counts[blockIdx.x];
  if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && buf[n - 1] != '\n') starts[rows] = n + 1;
#pragma unroll
  for (int it = 0; it < kTextLoadsPerThread; ++it) {
    const u32 i = t0 + it * kStep + threadIdx.x * kTextLoad;
    u32 m = newline_mask(buf, i, n, alloc);
    const u32 c = __builtin_popcount(m);
    u32 prefix = 0, wtot = 0;
#pragma unroll
    for (int b = 0; b < 5; ++b) {                              // c <= 16: five bits
      const u64 bal = __ballot((c >> b) & 1u);
      prefix += (u32)__builtin_popcountll(bal & lt) << b;
      wtot += (u32)__builtin_popcountll(bal) << b;
    }
    if (lane == 0) wc[it & 1][wave] = wtot;
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const u32 x = wc[it & 1][w];
      before += w < wave ? x : 0u;
      tot += x;
    }
    u32 k = base + before + prefix + 1;
    while (m) {
      const u32 bit = __builtin_ctz(m);
      m &= m - 1;
      if (k <= rows) starts[k] = i + bit + 1;
      ++k;
    }
    base += tot;
  }
}

// ------------------------------------------------------------------------------------------------ decode
// a lane's window on its row: the bytes from pos to the end of pos's aligned 16-byte block
struct Cursor {
  u64 lo, hi;
  u32 pos, left;
};

__device__ __forceinline__ void cursor_open(Cursor& c, const u8* __restrict__ buf, u32 s, u32 n, u32 alloc) {
  const W16 w = load16(buf, s & ~15u, n, alloc);
  const u32 k = s & 15u;
  c.lo = w.lo;
  c.hi = w.hi;
  if (k >= 8) {
    c.lo = w.hi >> (8 * (k - 8));
    c.hi = 0;
  } else if (k) {
    c.lo = (w.lo >> (8 * k)) | (w.hi << (64 - 8 * k));
    c.hi = w.hi >> (8 * k);
  }
  c.pos = s;
  c.left = 16 - k;
}

// the byte at pos (the caller has checked pos < the row's end <= n)
__device__ __forceinline__ u32 cursor_next(Cursor& c, const u8* __restrict__ buf, u32 n, u32 alloc) {
  if (c.left == 0) {
    const W16 w = load16(buf, c.pos, n, alloc);              // pos is a multiple of 16 here
    c.lo = w.lo;
    c.hi = w.hi;
    c.left = 16;
  }
  const u32 b = (u32)c.lo & 0xFFu;
  c.lo = (c.lo >> 8) | (c.hi << 56);
  c.hi >>= 8;
  ++c.pos;
  --c.left;
  return b;
}

__global__ __launch_bounds__(kTextThreads) void tp_decode_kernel(const u8* __restrict__ buf, u32 n, u32 alloc,
                                                                 const u32* __restrict__ starts, u32 rows,
                                                                 TextFields F, int nf, u32 delim, int trailing,
                                                                 u64* __restrict__ state, u64* __restrict__ list,
                                                                 u64 cap) {
  const u32 r = blockIdx.x * (u32)kTextThreads + threadIdx.x;
  if (r >= rows) return;
  const u32 s = starts[r];
  u32 e = starts[r + 1] - 1;
  if (e > n) e = n;                                           // whatever the index holds, nothing past the payload
  if (e > s && buf[e - 1] == '\r') --e;
  Cursor c;
  c.lo = c.hi = 0;
  c.pos = s;
  c.left = 0;
  if (s < e) cursor_open(c, buf, s, n, alloc);
  u32 err = 0;
  for (int f = 0; f < nf; ++f) {                              // wave-uniform: kind and pointer are scalar loads
    const u32 kind = F.kind[f];
    void* const out = F.out[f];
    const bool numeric = kind >= TEXT_INT && kind <= TEXT_DATE;
    const u32 fs = c.pos;
    bool closed = false;
    u64 mant = 0, scale = 1, w8 = 0;
    u32 nd = 0, nondig = 0, minus = 0, dots = 0, len = 0;
    while (c.pos < e) {
      const u32 b = cursor_next(c, buf, n, alloc);
      if (b == delim) {
        closed = true;
        break;
      }
      if (numeric) {
        const u32 bit = 1u << (len < 31 ? len : 31);
        const u32 d = b - 48u;
        if (d <= 9u) {
          mant = mant * 10 + d;
          ++nd;
          if (dots && nd <= 18) scale *= 10;
        } else {
          nondig |= bit;
          if (b == '-') minus |= bit;
          if (b == '.') dots = dots ? 0x80000000u | dots : bit;   // a second dot sets bit 31: never the grammar
        }
        if (len < 8) w8 |= (u64)b << (8 * len);
      }
      ++len;
    }
    const u32 fe = closed ? c.pos - 1 : c.pos;
    // structure: a delimiter after every field, or between fields only
    const bool want_closed = trailing || f + 1 < nf;
    if (closed != want_closed) {
      err = TEXT_ERR_ROW;
      break;
    }
    bool flag = false;
    if (kind == TEXT_INT) {
      const bool ok = len <= 20 && nd >= 1 && nd <= 18 && (nondig & ~1u) == 0 && (nondig & 1u) == (minus & 1u);
      flag = !ok;
      reinterpret_cast<i64*>(out)[r] = !ok ? 0 : (nondig & 1u) ? -(i64)mant : (i64)mant;
    } else if (kind == TEXT_FLOAT) {
      const u32 neg = nondig & minus & 1u;
      const bool ok = len <= 20 && nd >= 1 && nd <= 15 && (dots >> 31) == 0 && nondig == (neg | dots);
      flag = !ok;
      const double v = (double)mant / (double)scale;           // both exact: one IEEE division
      reinterpret_cast<double*>(out)[r] = !ok ? 0.0 : neg ? -v : v;
    } else if (kind == TEXT_BOOL) {
      const bool t = (len == 1 && w8 == 0x31ull) || (len == 4 && (w8 == 0x65757274ull || w8 == 0x65757254ull));
      const bool z = (len == 1 && w8 == 0x30ull) || (len == 5 && (w8 == 0x65736C6166ull || w8 == 0x65736C6146ull));
      flag = !(t || z);
      reinterpret_cast<u8*>(out)[r] = t ? 1 : 0;
    } else if (kind == TEXT_DATE) {
      const u32 dashes = (1u << 4) | (1u << 7);
      const bool ok = len == 10 && nd == 8 && nondig == dashes && minus == dashes;
      if (!ok && err == 0) err = TEXT_ERR_DATE;
      reinterpret_cast<int*>(out)[r] = ok ? (int)mant : 0;
    } else if (kind == TEXT_STR) {
      reinterpret_cast<i64*>(out)[r] = (i64)fs;
      reinterpret_cast<i64*>(out)[(u64)rows + r] = (i64)fe;
    }
    if (flag) {
      const u64 at = atomicAdd(&state[2], 1ull);
      if (list != nullptr && at < cap) {
        list[2 * at] = ((u64)r << 8) | (u64)f;
        list[2 * at + 1] = ((u64)fs << 32) | (u64)fe;
      }
    }
  }
  if (err != TEXT_ERR_ROW && c.pos != e) err = TEXT_ERR_ROW;   // bytes after the last field's delimiter
  if (err) atomicMin(&state[1], ((u64)r << 8) | (u64)err);
}

}  // namespace nsdb_text

extern "C" {

// The plan of a call as 8 numbers: rc, tile, tiles, scan_step, launches, counts_bytes, state_bytes, scratch_bytes.
int nsdb_textparse_plan(long long nbytes, int nfields, int delimiter, long long* f) {
  const nsdb::TextPlan p = nsdb::textparse_plan(nbytes, nfields, delimiter);
  f[0] = p.rc; f[1] = p.tile; f[2] = p.tiles; f[3] = p.scan_step; f[4] = p.launches; f[5] = p.counts_bytes;
  f[6] = p.state_bytes; f[7] = p.scratch_bytes;
  return p.rc;
}

// buf: 16-byte aligned, n payload bytes of an allocation of alloc >= n bytes. counts: plan.counts_bytes; state:
// plan.state_bytes. After it state[0] holds the row count.
int nsdb_textparse_index(const void* buf, long long n, long long alloc, int nfields, int delimiter, unsigned* counts,
                         unsigned long long* state, hipStream_t st) {
  using namespace nsdb_text;
  const nsdb::TextPlan p = nsdb::textparse_plan(n, nfields, delimiter);
  if (p.rc != nsdb::TEXT_OK || alloc < n || alloc >= (1ll << 31) + 16 || (reinterpret_cast<uintptr_t>(buf) & 15))
    return (int)hipErrorInvalidValue;
  const u8* b = reinterpret_cast<const u8*>(buf);
  hipLaunchKernelGGL(tp_count_kernel, dim3((unsigned)p.tiles), dim3(kTextThreads), 0, st, b, (u32)n, (u32)alloc, counts);
  hipLaunchKernelGGL(tp_scan_kernel, dim3(1), dim3(kTextThreads), 0, st, b, (u32)n, (u32)p.tiles, counts, state);
  return (int)hipGetLastError();
}

// rows: state[0] as read by the caller. kinds / outs: one per field of the file (outs[f]: [rows] int64 / float64 /
// uint8 / int32 by kind, [2, rows] int64 for a string field, unused for a skipped one). starts: rows + 1 u32, written
// when write_rows is set. list: cap pairs of u64 or null (cells are then only counted in state[2]).
int nsdb_textparse_decode(const void* buf, long long n, long long alloc, const unsigned char* kinds, void* const* outs,
                          int nfields, int delimiter, int trailing, long long rows, const unsigned* counts,
                          unsigned* starts, unsigned long long* state, unsigned long long* list, long long cap,
                          int write_rows, hipStream_t st) {
  using namespace nsdb_text;
  const nsdb::TextPlan p = nsdb::textparse_plan(n, nfields, delimiter);
  if (p.rc != nsdb::TEXT_OK || alloc < n || alloc >= (1ll << 31) + 16 || (reinterpret_cast<uintptr_t>(buf) & 15) ||
      rows < 1 || rows > n + 1)
    return (int)hipErrorInvalidValue;
  TextFields F{};
  for (int f = 0; f < nfields; ++f) {
    if (kinds[f] > nsdb::TEXT_STR || (kinds[f] != nsdb::TEXT_SKIP && outs[f] == nullptr)) return (int)hipErrorInvalidValue;
    F.kind[f] = kinds[f];
    F.out[f] = outs[f];
  }
  const u8* b = reinterpret_cast<const u8*>(buf);
  if (write_rows)
    hipLaunchKernelGGL(tp_rows_kernel, dim3((unsigned)p.tiles), dim3(kTextThreads), 0, st, b, (u32)n, (u32)alloc, counts,
                       (u32)rows, starts);
  hipLaunchKernelGGL(tp_decode_kernel, dim3((unsigned)((rows + kTextThreads - 1) / kTextThreads)), dim3(kTextThreads), 0,
                     st, b, (u32)n, (u32)alloc, (const u32*)starts, (u32)rows, F, nfields, (u32)delimiter, trailing, state,
                     list, (u64)(cap > 0 ? cap : 0));
  return (int)hipGetLastError();
}
}
