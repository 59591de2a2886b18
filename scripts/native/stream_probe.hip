// Operand-stream probe for the FF layer-1 GEMM (1000 x 1000 x 597568, 16 tiles x 16 splits = 256 workgroups): the
// A-side global -> LDS stream of gemm_nt_256_8ph_kernel alone (no MFMAs, no LDS reads), from three layouts of the
// same 1.2 GB operand:
//   row   row-major [rows][K] at pitch K: one k-tile of one row is a single 128-byte line, the kernel's own
//         lane-to-row map (every 1 KiB wave-instruction touches 8 rows, 1.2 MB apart)
//   pk8   packed [k-tile][Rp][64] read with the kernel's half-tile row sets (A0 = rows {0..63, 128..191},
//         A1 = {64..127, 192..255}): a half-tile is two 8 KiB runs, a k-tile of the tile one 32 KiB run
//   pk16  the same packed copy read as half-tiles of 128 consecutive rows: one 16 KiB run each
// 256 workgroups x 512 threads, workgroup -> (split, tile) as the kernel does it (xcd_remap + grouped walk), 16 B
// per lane LDS-DMA, three 16 KiB half-tiles in flight on a counted vmcnt. 20 timed launches per arm, interleaved.
//   hipcc -O3 --offload-arch=gfx950 scripts/native/stream_probe.hip -o stream_probe && ./stream_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef __attribute__((address_space(3))) void lds_void;
constexpr int OOB = 0x7ffffff0;   // voffset that the buffer range check turns into zeros
constexpr int BK = 64, HALF = 128 * 128, GROUP_M = 8;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  if (nwg <= 8) return bid;
  const int xcd = bid & 7, pos = bid >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}
__device__ __forceinline__ void grouped_tile(int tile, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int per_group = GROUP_M * tiles_n;
  const int g = tile / per_group;
  const int first_m = g * GROUP_M;
  const int gsize = min(tiles_m - first_m, GROUP_M);
  const int r = tile - g * per_group;
  tm = first_m + r % gsize;
  tn = r / gsize;
}

struct ProbeParams {
  const unsigned short* A;    // row-major [M][lda]
  const unsigned short* P;    // packed [KT][Rp][64]
  unsigned* out;
  long long lda;
  int M, K, kchunk, tiles_m, tiles_n, splits, Rp, KT;
};

// MODE 0 row, 1 pk8, 2 pk16
template <int MODE>
__global__ void __launch_bounds__(512, 2) stream_probe_kernel(ProbeParams p) {
  // the ring is the first 48 KiB; sized like the GEMM's LDS (137 KiB) so that, as there, one workgroup runs per CU
  __shared__ __attribute__((aligned(16))) char smem[8 * HALF + 9 * 1024];
  const int ntiles = p.tiles_m * p.tiles_n;
  const int wg = xcd_remap(blockIdx.x, ntiles * p.splits);
  const int split = wg / ntiles, tile = wg % ntiles;
  int tm, tn;
  grouped_tile(tile, p.tiles_m, p.tiles_n, tm, tn);
  const int m0 = tm * 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows_a = min(256, p.M - m0);
  const int kbeg = split * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  const int nk = max(0, (kend - kbeg + BK - 1) / BK);
  const int nh = 2 * nk;     // half-tiles to stream
  const int kt0 = kbeg / BK;

  const int lr = wave * 8 + (lane >> 3);
  const int kc = ((lane & 7) ^ ((lr >> 1) & 7)) * 8;
  int roff[2][2];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ta = MODE == 2 ? q * 128 + i * 64 + lr : i * 128 + q * 64 + lr;   // row of the tile
      if constexpr (MODE == 0) roff[q][i] = ta < rows_a ? (int)((long long)ta * p.lda * 2) : -1;
      else roff[q][i] = (ta * 64 + kc) * 2;
    }
  const __amdgpu_buffer_rsrc_t ra =
      MODE == 0 ? make_rsrc(p.A + (long long)m0 * p.lda, (unsigned)((long long)rows_a * p.lda * 2))
                : make_rsrc(p.P, (unsigned)((long long)p.KT * p.Rp * 128));

  auto stage = [&](int slot, int h) {
    const int u = h >> 1, q = h & 1;
    char* dst = smem + slot * HALF;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if constexpr (MODE == 0) {
        const int k = kbeg + u * BK + kc;
        const int ro = roff[q][i];
        const int voff = (k < kend && ro >= 0) ? ro + k * 2 : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(dst + (i * 64 + wave * 8) * 128), 16, voff, 0, 0, 0);
      } else {
        const unsigned soff = ((unsigned)(kt0 + u) * p.Rp + m0) * 128u;   // wave-uniform, < 2^32 (host-checked)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void*)(dst + (i * 64 + wave * 8) * 128), 16, roff[q][i],
                                                 (int)soff, 0, 0);
      }
    }
  };

  int slot = 0;
  for (int h = 0; h < 3 && h < nh; ++h) stage(h, h);
  for (int h = 0; h < nh; ++h) {
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // the oldest of the three half-tiles in flight has landed
    if (h + 3 < nh) stage(slot, h + 3);
    slot = slot == 2 ? 0 : slot + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // one dependent read of the ring so the stream has a consumer
  const unsigned v = reinterpret_cast<const unsigned*>(smem)[tid];
  if (v == 0x12345678u && p.out) p.out[blockIdx.x] = v;
}

__global__ void fill_kernel(unsigned* a, long long n, unsigned seed) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    unsigned long long z = seed + (unsigned long long)i * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    // two bf16 in [-2, 2): random sign and mantissa, exponent 126..127
    const unsigned lo = (unsigned)(z >> 8) & 0x80ffu, hi = (unsigned)(z >> 32) & 0x80ffu;
    a[i] = (lo | 0x3f00u) | ((hi | 0x3f00u) << 16);
  }
}

// packed[kt][r][c] = A[r][64 kt + c], zero outside rows x K; 16 B per thread
__global__ void pack_kernel(const unsigned short* A, uint4* P, long long lda, int M, int K, int Rp, int KT) {
  const long long n = (long long)KT * Rp * 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c8 = (int)(i & 7);
    const long long rr = i >> 3;
    const int r = (int)(rr % Rp), kt = (int)(rr / Rp);
    const int k = kt * 64 + c8 * 8;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < M && k + 8 <= K) v = *reinterpret_cast<const uint4*>(A + (long long)r * lda + k);
    P[i] = v;
  }
}

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

int main() {
  ProbeParams p{};
  p.M = 1000; p.K = 597568; p.lda = p.K; p.tiles_m = 4; p.tiles_n = 4; p.splits = 16;
  p.kchunk = 37376;                         // the plan's K share: 584 k-tiles (the last split has 577)
  p.KT = (p.K + 63) / 64; p.Rp = 1024;
  if (p.K % 8 != 0) return 1;
  const long long a_bytes = (long long)p.M * p.lda * 2, p_bytes = (long long)p.KT * p.Rp * 128;
  if (p_bytes >= (1ll << 32) - 16) return 1;
  unsigned short *dA, *dP;
  CHECK(hipMalloc(&dA, a_bytes));
  CHECK(hipMalloc(&dP, p_bytes));
  CHECK(hipMalloc(&p.out, 256 * 4));
  p.A = dA; p.P = dP;
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, (unsigned*)dA, a_bytes / 4, 7u);
  hipLaunchKernelGGL(pack_kernel, dim3(4096), dim3(256), 0, 0, dA, (uint4*)dP, p.lda, p.M, p.K, p.Rp, p.KT);
  CHECK(hipDeviceSynchronize());

  // bytes the 256 workgroups ask for (each A tile is streamed by the 4 column tiles of its row) and unique bytes
  const double req = 4.0 * (double)p.M * p.K * 2, uniq = (double)p.M * p.K * 2;
  const int NL = 20, NARM = 3;
  const char* name[NARM] = {"row ", "pk8 ", "pk16"};
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  auto launch = [&](int arm) {
    if (arm == 0) hipLaunchKernelGGL(stream_probe_kernel<0>, dim3(256), dim3(512), 0, 0, p);
    else if (arm == 1) hipLaunchKernelGGL(stream_probe_kernel<1>, dim3(256), dim3(512), 0, 0, p);
    else hipLaunchKernelGGL(stream_probe_kernel<2>, dim3(256), dim3(512), 0, 0, p);
  };
  std::vector<float> ms[NARM];
  for (int rep = -3; rep < NL; ++rep)       // 3 untimed warm-up rounds
    for (int arm = 0; arm < NARM; ++arm) {
      CHECK(hipEventRecord(e0));
      launch(arm);
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float t = 0.f;
      CHECK(hipEventElapsedTime(&t, e0, e1));
      if (rep >= 0) ms[arm].push_back(t);
    }
  CHECK(hipGetLastError());
  float med[NARM], lo[NARM], hi[NARM];
  for (int arm = 0; arm < NARM; ++arm) {
    std::vector<float> s = ms[arm];
    std::sort(s.begin(), s.end());
    med[arm] = 0.5f * (s[NL / 2 - 1] + s[NL / 2]); lo[arm] = s.front(); hi[arm] = s.back();
    printf("%s: ms median %.4f min %.4f max %.4f | requested TB/s median %.3f best %.3f | unique (HBM-side) TB/s median %.3f best %.3f\n",
           name[arm], med[arm], lo[arm], hi[arm], req / (med[arm] * 1e-3) / 1e12, req / (lo[arm] * 1e-3) / 1e12,
           uniq / (med[arm] * 1e-3) / 1e12, uniq / (lo[arm] * 1e-3) / 1e12);
  }
  const float spread = hi[0] - lo[0];
  printf("row-major spread (max - min over %d launches): %.4f ms\n", NL, spread);
  for (int arm = 1; arm < NARM; ++arm)
    printf("%s vs row: median gain %.4f ms = %.2f x spread -> gate (> 2 x spread) %s\n", name[arm], med[0] - med[arm],
           spread > 0 ? (med[0] - med[arm]) / spread : 0.f, med[0] - med[arm] > 2 * spread ? "PASS" : "FAIL");
  return 0;
}
