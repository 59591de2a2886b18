// Launch plan of the device ORDER BY (sort.hip): plain C++17, no HIP, so the host compiler alone builds it
// (tests/native/sort_plan_dump.cpp). sort_plan maps (key dtypes, n) to everything the launcher and the binding need:
// the launcher launches what it says, the binding sizes every allocation from it. Nothing here depends on the data.
#pragma once

namespace nsdb {

constexpr int kSortMaxKeys = 4;
constexpr int kSortBins = 256;            // 8-bit digits
constexpr int kSortThreads = 256;
constexpr int kSortRowsPerThread = 16;
constexpr int kSortTile = kSortThreads * kSortRowsPerThread;   // rows ranked by one scatter workgroup
constexpr int kSortScanStep = kSortThreads;                    // tiles one os_scan_kernel workgroup covers in one step
constexpr int kSortSlots = 32;            // digit slots: key j, byte b -> 8 j + b
constexpr int kSortHistGridCap = 1024;
constexpr int kSortHistRows = kSortThreads * 4;                // rows one os_hist_kernel workgroup takes per step
// state layout in u32 words: hist[32][256] | base[32][256] | per slot: live, live passes before it, write-words |
// per key: live | live passes in all
constexpr int kSortHistOff = 0;
constexpr int kSortBaseOff = kSortSlots * kSortBins;
constexpr int kSortLiveOff = 2 * kSortSlots * kSortBins;
constexpr int kSortBeforeOff = kSortLiveOff + kSortSlots;
constexpr int kSortWriteOff = kSortBeforeOff + kSortSlots;
constexpr int kSortKeyLiveOff = kSortWriteOff + kSortSlots;
constexpr int kSortTotalOff = kSortKeyLiveOff + kSortMaxKeys;
constexpr int kSortStateWords = kSortTotalOff + 4;

enum { SORT_OK = 0, SORT_BAD_M = -1, SORT_BAD_DTYPE = -2, SORT_BAD_N = -3 };

struct SortPlan {
  int rc;                  // SORT_OK or the first failed check
  int word_bits;           // 32 when every key is 4 bytes wide, otherwise 64
  int tile;                // rows per tile
  long long tiles;         // T
  int passes;              // sum of the key bytes: one count / scan / scatter triple each, live or not
  int launches;            // hist + plan + one load per key + 3 per pass + out
  int scan_step;           // tiles per os_scan_kernel step
  int hist_grid;           // workgroups of os_hist_kernel
  long long state_bytes;   // zeroed by the caller
  long long counts_bytes;  // [256][T] u32
  long long words_bytes;   // 2 buffers of n order words
  long long ids_bytes;     // 2 buffers of n u32 row ids
  long long scratch_bytes; // the four together
};

// bytes of a key of dtype code dt (0 int32, 1 float32, 2 int64, 3 float64)
inline int sort_key_bytes(int dt) { return dt == 0 || dt == 1 ? 4 : 8; }

inline SortPlan sort_plan(const int* dt, int m, long long n) {
  SortPlan p{};
  if (m < 1 || m > kSortMaxKeys) {
    p.rc = SORT_BAD_M;
    return p;
  }
  p.word_bits = 32;
  for (int j = 0; j < m; ++j) {
    if (dt[j] < 0 || dt[j] > 3) {
      p.rc = SORT_BAD_DTYPE;
      return p;
    }
    p.passes += sort_key_bytes(dt[j]);
    if (sort_key_bytes(dt[j]) == 8) p.word_bits = 64;
  }
  if (n < 1 || n >= (1ll << 31)) {
    p.rc = SORT_BAD_N;
    return p;
  }
  p.tile = kSortTile;
  p.tiles = (n + kSortTile - 1) / kSortTile;
  p.launches = 2 + m + 3 * p.passes + 1;
  p.scan_step = kSortScanStep;
  const long long hg = (n + kSortHistRows - 1) / kSortHistRows;
  p.hist_grid = (int)(hg < kSortHistGridCap ? hg : kSortHistGridCap);
  p.state_bytes = 4ll * kSortStateWords;
  p.counts_bytes = 4ll * kSortBins * p.tiles;
  p.words_bytes = 2 * n * (p.word_bits / 8);
  p.ids_bytes = 2 * n * 4;
  p.scratch_bytes = p.state_bytes + p.counts_bytes + p.words_bytes + p.ids_bytes;
  return p;
}

}  // namespace nsdb
