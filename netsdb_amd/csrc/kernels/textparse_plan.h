// Launch plan of the delimited-text parser (textparse.hip): plain C++17, no HIP, so the host compiler alone builds it
// (tests/native/textparse_plan_dump.cpp). textparse_plan maps (buffer bytes, fields per row, delimiter) to everything
// the launcher and the binding need before the data is seen: the launcher launches what it says, the binding sizes the
// scratch from it. The two allocations that depend on the data (the row index and the flagged-cell list) are sized by
// textparse_rows_bytes / textparse_flags_bytes from the counts the kernels report.
#pragma once

namespace nsdb {

constexpr int kTextThreads = 256;
constexpr int kTextLoad = 16;                                // bytes per load
constexpr int kTextLoadsPerThread = 4;
constexpr int kTextTile = kTextThreads * kTextLoad * kTextLoadsPerThread;   // 16 KiB scanned by one workgroup
constexpr int kTextScanStep = kTextThreads;                  // tiles one tp_scan_kernel step covers
constexpr int kTextMaxFields = 64;
constexpr int kTextStateWords = 4;                           // u64: rows | lowest bad (row << 8 | code) | flagged | 0

// field kinds, one per column of the file
enum { TEXT_SKIP = 0, TEXT_INT = 1, TEXT_FLOAT = 2, TEXT_BOOL = 3, TEXT_DATE = 4, TEXT_STR = 5 };
// error codes in the low byte of the bad-row word
enum { TEXT_ERR_ROW = 1, TEXT_ERR_DATE = 2 };

enum { TEXT_OK = 0, TEXT_EMPTY = -1, TEXT_TOO_LARGE = -2, TEXT_BAD_NFIELDS = -3, TEXT_BAD_DELIM = -4 };

struct TextPlan {
  int rc;                   // TEXT_OK or the first failed check
  int tile;                 // bytes per tile
  long long tiles;          // ceil(nbytes / tile)
  int scan_step;            // tiles per scan step
  int launches;             // count, scan, rows, decode
  long long counts_bytes;   // [tiles] u32: newlines per tile, then their exclusive scan
  long long state_bytes;    // kTextStateWords u64
  long long scratch_bytes;  // the two together
};

inline long long textparse_rows_bytes(long long rows) { return 4 * (rows + 1); }   // u32 row starts, one past the end
inline long long textparse_flags_bytes(long long cells) { return 16 * cells; }     // (row << 8 | field, start << 32 | end)

inline TextPlan textparse_plan(long long nbytes, int nfields, int delimiter) {
  TextPlan p{};
  if (nbytes < 1) {
    p.rc = TEXT_EMPTY;
    return p;
  }
  if (nbytes >= (1ll << 31)) {
    p.rc = TEXT_TOO_LARGE;
    return p;
  }
  if (nfields < 1 || nfields > kTextMaxFields) {
    p.rc = TEXT_BAD_NFIELDS;
    return p;
  }
  if (delimiter < 0 || delimiter > 255 || delimiter == '\n' || delimiter == '\r') {
    p.rc = TEXT_BAD_DELIM;
    return p;
  }
  p.tile = kTextTile;
  p.tiles = (nbytes + kTextTile - 1) / kTextTile;
  p.scan_step = kTextScanStep;
  p.launches = 4;
  p.counts_bytes = 4 * p.tiles;
  p.state_bytes = 8ll * kTextStateWords;
  p.scratch_bytes = p.counts_bytes + p.state_bytes;
  return p;
}

}  // namespace nsdb
