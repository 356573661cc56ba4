// dtk_decimal.h -- decimal integers as strconv.Itoa writes them: the renderers' position lines (dtk_render.hip,
// dtk_streampos.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t dec_len(int32_t v) {
  const uint32_t neg = v < 0 ? 1u : 0u;
  const uint32_t u = neg ? (uint32_t)(-(int64_t)v) : (uint32_t)v;
  return 1u + (u >= 10u) + (u >= 100u) + (u >= 1000u) + (u >= 10000u) + (u >= 100000u) + (u >= 1000000u) +
         (u >= 10000000u) + (u >= 100000000u) + (u >= 1000000000u) + neg;
}

__device__ __forceinline__ void dec_put(uint8_t *o, int32_t v, uint32_t n) {
  uint32_t u = v < 0 ? (uint32_t)(-(int64_t)v) : (uint32_t)v;
  uint32_t i = n;
  do { o[--i] = (uint8_t)('0' + u % 10u); u /= 10u; } while (u != 0u && i > 0u);
  if (v < 0) o[0] = '-';
}

// the same for Go's 64-bit int: a stream's posC runs across slices (dtk_streampos.hip)
__device__ __forceinline__ uint32_t dec_len64(int64_t v) {
  uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  uint32_t n = v < 0 ? 2u : 1u;
  for (uint64_t p = 10ull; u >= p; p *= 10ull) n++;  // (u < 2^63 < 10^19: p stays below 2^64)
  return n;
}

// writes the n = dec_len64(v) bytes of v at o, none of them at or behind `cap`
__device__ __forceinline__ void dec_put64(uint8_t *out, uint64_t o, uint64_t cap, int64_t v, uint32_t n) {
  uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  uint32_t i = n;
  do {
    --i;
    if (o + i < cap) out[o + i] = (uint8_t)('0' + (uint32_t)(u % 10ull));
    u /= 10ull;
  } while (u != 0ull && i > 0u);
  if (v < 0 && o < cap) out[o] = '-';
}
