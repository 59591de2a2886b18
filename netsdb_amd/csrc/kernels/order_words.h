// Order words of the device ORDER BY kernels (topk.hip: ORDER BY ... LIMIT k; sort.hip: the full ORDER BY). Every key
// element maps in registers to an unsigned order word (32 significant bits for 4-byte keys, 64 for 8-byte ones) whose
// unsigned order is the contract's order: signed ints flip the sign bit; floats fold -0.0 into +0.0, map every NaN to
// the top word (above +inf) and take the sign-magnitude flip; a descending key is complemented. Columns are read in
// their native width. Included inside the including file's own namespace, after its u32 / u64 / i64 typedefs and
// kMaxKeys.
#pragma once

enum { DT_I32 = 0, DT_F32 = 1, DT_I64 = 2, DT_F64 = 3 };

struct Keys {
  const void* p[kMaxKeys];
  int dt[kMaxKeys];
  int desc[kMaxKeys];
  int m;
  int idbits;     // significant bits of the largest row id (>= 1)
};

__device__ __forceinline__ u64 word_at(const void* p, int dt, int desc, i64 i) {
  if (dt == DT_I32 || dt == DT_F32) {
    u32 b = reinterpret_cast<const u32*>(p)[i];
    if (dt == DT_I32) {
      b ^= 0x80000000u;
    } else {
      const u32 mag = b & 0x7FFFFFFFu;
      if (mag == 0) b = 0;                                   // -0.0 == +0.0
      b = mag > 0x7F800000u ? 0xFFFFFFFFu : ((b >> 31) ? ~b : (b | 0x80000000u));
    }
    return desc ? (u64)(~b) : (u64)b;
  }
  u64 b = reinterpret_cast<const u64*>(p)[i];
  if (dt == DT_I64) {
    b ^= 0x8000000000000000ull;
  } else {
    const u64 mag = b & 0x7FFFFFFFFFFFFFFFull;
    if (mag == 0) b = 0;
    b = mag > 0x7FF0000000000000ull ? ~0ull : ((b >> 63) ? ~b : (b | 0x8000000000000000ull));
  }
  return desc ? ~b : b;
}

// key j's order word of row i (j a run-time value: selected by compares, never an indexed private copy of K)
__device__ __forceinline__ u64 key_word(const Keys& K, int j, i64 i) {
  const void* p = K.p[0];
  int dt = K.dt[0], desc = K.desc[0];
#pragma unroll
  for (int t = 1; t < kMaxKeys; ++t)
    if (j == t) {
      p = K.p[t];
      dt = K.dt[t];
      desc = K.desc[t];
    }
  return word_at(p, dt, desc, i);
}
