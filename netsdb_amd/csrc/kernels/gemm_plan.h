// Launch plan of the block GEMM (gemm.hip): the ONE place that turns a call (shape, strides, options) into a
// launch — tile config, split-K partition, workgroups, epilogue, kernel, reducer. The launcher fills GemmParams from
// the plan and switches on it; the bindings size the workspace from it; ops.gemm_plan shows it to tests and callers.
// Plain C++17 (no HIP, no torch): a host compiler builds it alone (tests/native/gemm_plan_dump.cpp).
#pragma once
#include <algorithm>

namespace nsdb {

constexpr int BM = 128, BN = 128, BK = 64;       // the general tile and the k-tile of every GEMM kernel
constexpr int BT256 = 256;                       // the 8-phase macro tile (and the long side of the stream tiles)

enum GemmKernel { GEMM_TILE128, GEMM_8PH, GEMM_8PH32, GEMM_8PH_FIXUP, GEMM_STREAM256X128, GEMM_STREAM128X256,
                  GEMM_8PH_PK };
enum GemmReducer { GEMM_REDUCE_NONE, GEMM_REDUCE_PLAIN, GEMM_REDUCE_WIDE, GEMM_REDUCE_IN_LAUNCH };

inline const char* gemm_kernel_name(int k) {
  static const char* const names[] = {"tile128", "8ph", "8ph32", "8ph_fixup", "stream256x128", "stream128x256",
                                      "8ph_pk"};
  return k >= 0 && k < 7 ? names[k] : "?";
}
inline const char* gemm_reducer_name(int r) {
  static const char* const names[] = {"none", "plain", "wide", "in_launch"};
  return r >= 0 && r < 4 ? names[r] : "?";
}

// What the caller asks for. The options are requests: the plan says what each became.
struct GemmCall {
  int M = 0, N = 0, K = 0, batch = 1;
  int splits = 0;            // requested split-K slices; <= 0: the library's choice
  int cfg = -1;              // -1 auto, 0 = 128x128 tile, 2 = 256x256 8-phase, 3 / 4 = 256x128 / 128x256 stream
  int epi = -1;              // 8-phase unsplit epilogue: -1 auto (direct), 0 LDS-staged, 1 direct register stores
  int mfma = 0;              // 8-phase main loop: 0 auto, 16 = 16x16x32, 32 = 32x32x16 (direct epilogue launches)
  int fixup = 0;             // 8-phase split-K: 1 = reduce inside the launch (the caller has the fix-up state)
  int kinter = 0;            // stream tiles: 1 = k-interleaved splits (split s takes k-tiles s, s + S, ...)
  int out_f32 = 0, accumulate = 0;
  int bias_mode = 0;         // 0 when there is no bias
  long long lda = 0, ldb = 0, ldc = 0, sC = 0;
  int c_align = 16;          // alignment of the C pointer in bytes (gemm_ptr_align)
  long long seg_k = 0;       // K-segmented B: segment length (0: plain B)
  int has_ws = 1;            // a split-K workspace is (or will be) there
  int packed = 0;            // 8-phase: 1 / 2 = the caller also has A / B as its k-tile-major copy (ops.pack_ktile)
};

struct GemmPlan {
  int rc = 0;                // 0, or the first failed check: -1 16-B rows (K, lda, ldb % 8), -2 per-tile buffer range,
                             // -3 split-K without a workspace, -4 accumulate into bf16, -8 not a production config,
                             // -5 a split crosses a K segment. The geometry below is filled either way.
  int cfg = 0, tbm = 0, tbn = 0, tiles_m = 0, tiles_n = 0;
  int splits = 1;            // effective: every split owns kchunk of K, the last one the remainder
  int kchunk = 0;
  long long wgs = 0;         // workgroups of the launch (grid x * z); 0: an empty GEMM, nothing is launched
  int vec_ws = 0, vec_c = 0, direct_epi = 0;
  int kernel = GEMM_TILE128;
  int kinter = 0;            // effective
  int reducer = GEMM_REDUCE_NONE;
  int reduce_blocks = 0;     // grid x of the reducer launch (grid y = batch)
  int prefetch_eligible = 0;
  int packed = 0;            // effective: the operand (1 = A, 2 = B) the launch streams from its packed copy
};

// Bytes of the k-tile-major packed copy of a [rows, K] operand: [ceil(K / 64)][rows rounded up to 256][64] bf16.
inline long long packed_rows(long long rows) { return (rows + BT256 - 1) / BT256 * BT256; }
inline long long packed_bytes(long long rows, long long K) { return (K + BK - 1) / BK * packed_rows(rows) * BK * 2; }


// Alignment of a pointer in bytes, as far as the plan cares (16 at most).
inline int gemm_ptr_align(const void* p) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(p) | 16;
  return (int)(a & (~a + 1));
}

// Tile config: the 256x256 8-phase tile (1 block/CU) when both dims fill it and there is enough work.
inline int pick_cfg(int M, int N, int K, int batch) {
  const long long big_tiles = (long long)((M + 255) / 256) * ((N + 255) / 256) * batch;
  const bool fills = M >= 192 && N >= 192;
  const long long ksteps = (K + BK - 1) / BK;
  // 8-phase 256^2 when there is a long mainloop, or when >= 3/4 of the CUs get a tile and K spans at
  // least 16 k-tiles (the FF output layer 1000x14588x1000: 60 us vs 75 us for 128^2, kernel trace)
  if (fills && (big_tiles * ksteps >= 256LL * 32 || (big_tiles >= 192 && ksteps >= 16))) return 2;
  // skinny, very long K (the dedup scoring GEMMs 500 x 100 x 900k and 12 x 500 x 100 x 100k): memory-bound; the
  // 8-phase kernel keeps three half-tiles of A in flight and zero-fills the missing B rows without reading them
  // (common panel 205 vs 222 us, batched private panels 263 vs 285 us, profiles/r4_dedup)
  // skinny (one side <= 128 rows) with a long K: the 256x128 / 128x256 stream tile (MFMA work padded to 128, not
  // 256 rows; 2 k-tiles in flight per CU): 500x100x900k 208.7 vs 213.9 us, 12x500x100x100k 290.5 vs 292.9,
  // 4096x128x16k 38.4 vs 40.7 (8-phase) / 43.8 (128^2) (profiles/r5_stream)
  if (std::max(M, N) >= 192 && std::min(M, N) <= 128 && ksteps >= 256) return M >= N ? 3 : 4;
  if ((M >= 192 || N >= 192) && std::min(M, N) >= 64 && ksteps >= 1024) return 2;
  return 0;
}

// Macro tile of a config: 0 = 128x128, 2 = 256x256 8-phase, 3 = 256x128 stream, 4 = 128x256 stream.
inline void cfg_tile(int cfg, int& tbm, int& tbn) {
  tbm = cfg == 2 || cfg == 3 ? BT256 : BM;
  tbn = cfg == 2 || cfg == 4 ? BT256 : BN;
}

// Split-K slices the library picks for `tiles` workgroup tiles (batch included) of config `cfg` over `ksteps` k-tiles.
inline int auto_splits(int cfg, int tiles, int ksteps) {
  // fill the chip: 256 CUs x (2 blocks of 128^2 | 1 block of 256^2); keep >= 8 k-steps per split
  const int target = cfg ? 256 : 512;   // the 256^2 and stream tiles run one block per CU
  int splits = 1;
  // >= 3/4 of the chip busy: a split's f32 slabs + reduce pass cost more than the idle CUs (1000x14588x1024:
  // 51 us + 24 us reduce with 2 splits vs 60 us unsplit)
  if (tiles < target && !(cfg == 2 && tiles >= 192)) {
    // round DOWN: tiles * splits stays within one wave of resident workgroups. Rounding up left a
    // handful of workgroups for a second, nearly empty wave (6000x100x100k: 47 tiles x 11 splits =
    // 517 WGs ran 456 us; x 10 = 470 WGs fit one wave)
    splits = std::max(1, target / tiles);
    splits = std::min(splits, std::max(1, ksteps / 8));
  }
  if (splits > 1) {
    const int kchunk_steps = (ksteps + splits - 1) / splits;
    splits = (ksteps + kchunk_steps - 1) / kchunk_steps;
  }
  return splits;
}

inline GemmPlan gemm_plan(const GemmCall& c) {
  GemmPlan p;
  if (c.M <= 0 || c.N <= 0 || c.batch <= 0) return p;
  auto fail = [&p](int rc) { if (p.rc == 0) p.rc = rc; };
  if (c.K % 8 != 0 || c.lda % 8 != 0 || c.ldb % 8 != 0) fail(-1);      // 16-B rows for the LDS-DMA
  if (256LL * c.lda * 2 >= 0x7ffffff0LL || 256LL * c.ldb * 2 >= 0x7ffffff0LL) fail(-2);   // per-tile buffer range

  p.cfg = c.cfg < 0 ? pick_cfg(c.M, c.N, c.K, c.batch) : c.cfg;
  cfg_tile(p.cfg, p.tbm, p.tbn);
  p.tiles_m = (c.M + p.tbm - 1) / p.tbm;
  p.tiles_n = (c.N + p.tbn - 1) / p.tbn;
  const int tiles = p.tiles_m * p.tiles_n;
  const int ksteps = (c.K + BK - 1) / BK;
  // the requested (or chosen) count rounds to whole k-tiles per split; splits left without a k-tile are dropped
  const int want = c.splits > 0 ? c.splits : auto_splits(p.cfg, tiles * c.batch, ksteps);
  const int kchunk_steps = std::max(1, (ksteps + want - 1) / want);
  p.kchunk = kchunk_steps * BK;
  p.splits = std::max(1, (ksteps + kchunk_steps - 1) / kchunk_steps);
  p.wgs = (long long)tiles * p.splits * c.batch;

  if (p.splits > 1 && !c.has_ws) fail(-3);
  if (c.accumulate && !c.out_f32) fail(-4);                             // C += A.B^T only into f32
  if (p.cfg < 0 || p.cfg > 4 || p.cfg == 1) fail(-8);                   // not a production config
  if (c.seg_k > 0 && (c.seg_k % p.kchunk != 0 || c.seg_k % BK != 0)) fail(-5);   // a split must not cross a segment

  p.vec_ws = (c.N % 4 == 0) ? 1 : 0;
  p.vec_c = (c.ldc % 4 == 0 && c.sC % 4 == 0 && c.c_align % (c.out_f32 ? 16 : 8) == 0) ? 1 : 0;
  // the direct register epilogue for unsplit 8-phase launches with aligned C rows and for split-K slabs (epi:
  // -1 auto = direct, 0 = LDS-staged, 1 = direct); C += A.B^T and per-element bias keep the LDS-staged epilogue;
  // split-K slabs (N % 4 == 0) take the direct stores too
  p.direct_epi = (p.cfg == 2 && c.epi != 0 &&
                  ((p.splits == 1 && !c.accumulate && p.vec_c && c.bias_mode != 3) || (p.splits > 1 && p.vec_ws))) ? 1 : 0;

  const long long MN = (long long)c.M * c.N;
  if (p.cfg == 2) {
    // In-launch split-K reduction only where the separate reducer would be the plain one (same summation order:
    // bit-identical results); narrow outputs with many splits keep splitk_reduce_wide_kernel.
    const long long fx_blocks = (MN / 4 + 255) / 256;
    const bool fix = c.fixup && p.splits > 1 && p.splits <= 32 && p.direct_epi && p.vec_ws && c.batch == 1 &&
                     c.mfma != 32 && !(p.splits >= 8 && fx_blocks < 512);
    // the 32x32x16 main loop stores from registers only (store_direct_8ph32): launches that need the LDS-staged
    // epilogue (C += A.B^T, a per-element bias, unaligned C) stay on the 16x16x32 loop
    p.kernel = fix ? GEMM_8PH_FIXUP : (c.mfma == 32 && p.direct_epi) ? GEMM_8PH32 : GEMM_8PH;
  } else if (p.cfg == 3 || p.cfg == 4) {
    // contiguous K chunks per split; k-interleaved splits on request (unsegmented B only: a split must stay inside
    // one segment). A/B in profiles/r5_stream: interleaving wins 3 % at M = 1000, N <= 128 and loses 4-5 % on the
    // batched dedup panels, so it is not the default.
    p.kernel = p.cfg == 3 ? GEMM_STREAM256X128 : GEMM_STREAM128X256;
    p.kinter = (c.seg_k == 0 && p.splits > 1 && c.kinter) ? 1 : 0;
  }

  // A packed operand is streamed only by the plain 16x16x32 8-phase launch (common epilogue, separate reducer) of an
  // unbatched, unsegmented call, and only when one 32-bit buffer covers the copy with room for the out-of-range
  // offset behind it; otherwise the request is dropped and the launch reads the row-major operand.
  if ((c.packed == 1 || c.packed == 2) && p.kernel == GEMM_8PH && p.cfg == 2 && c.mfma != 32 && c.seg_k == 0 &&
      c.batch == 1 && packed_bytes(c.packed == 1 ? c.M : c.N, c.K) < (1LL << 32) - 16) {
    p.kernel = GEMM_8PH_PK;
    p.packed = c.packed;
  }

  if (p.kernel == GEMM_8PH_FIXUP) {
    p.reducer = GEMM_REDUCE_IN_LAUNCH;
  } else if (p.splits > 1) {
    // narrow outputs with many splits: the plain reducer has too few workgroups (splitk_reduce_wide_kernel)
    const long long plain_blocks = ((p.vec_ws ? MN / 4 : MN) + 255) / 256;
    const bool wide = p.vec_ws && p.splits >= 8 && plain_blocks * c.batch < 512;
    p.reducer = wide ? GEMM_REDUCE_WIDE : GEMM_REDUCE_PLAIN;
    p.reduce_blocks = wide ? (int)((MN / 4 + 63) / 64) : (int)std::min<long long>(plain_blocks, 4096);
  }
  // An operand prefetch is taken by an 8-phase launch of >= 128 workgroups with >= 64 k-tiles per workgroup: a long,
  // one-wave-resident GEMM whose finishing workgroups can warm the next operand.
  p.prefetch_eligible = (p.cfg == 2 && p.wgs >= 128 && kchunk_steps >= 64) ? 1 : 0;
  return p;
}

}  // namespace nsdb
