// Stand-in for <hip/hip_runtime.h> when tools/hram_lane_san.cpp compiles nw_sha512.hpp for the
// CPU: the HIP qualifiers as nothing, and the two gfx950 builtins the SHA-512 code uses as plain
// functions (v_alignbit_b32: the low 32 bits of (hi:lo) >> (sh & 31); v_bitop3_b32: bit by bit
// through the truth table, index (x << 2) | (y << 1) | z).
#pragma once
#include <stdint.h>
#define __device__
#define __host__
#define __global__
#define __constant__
#define __restrict__
#define __forceinline__ inline
static inline uint32_t nw_san_alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31));
}
static inline uint32_t nw_san_bitop3(uint32_t x, uint32_t y, uint32_t z, int lut) {
  uint32_t r = 0;
  for (int b = 0; b < 32; ++b) {
    const int idx = (int)((((x >> b) & 1u) << 2) | (((y >> b) & 1u) << 1) | ((z >> b) & 1u));
    r |= (uint32_t)((lut >> idx) & 1) << b;
  }
  return r;
}
#define __builtin_amdgcn_alignbit nw_san_alignbit
#define __builtin_amdgcn_bitop3_b32 nw_san_bitop3
