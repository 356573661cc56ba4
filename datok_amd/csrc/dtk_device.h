// dtk_device.h -- what the kernel units share: the wave helpers (scans, folds, the sum), one block scan of 256 threads
// per width and the in-place row scans on top of it, the searches, the list reads of a stream slice's units, the U+FFFD rule of
// the two renderers (which bytes print as the replacement character, how a surface is written with them expanded) and
// the per-document repair step (used by the verification's fix kernel and by the one-launch scan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dtk_decimal.h"
#include "dtk_internal.h"

#define WAVE 64
#ifndef DTK_WARM_TAG
#define DTK_WARM_TAG 64u
#endif  // how far behind a warm-up start an opening angle bracket is looked for

// ------------------------------------------------------------------ helpers

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & (WAVE - 1); }
__device__ __forceinline__ unsigned long long lanemask_lt() { return (1ull << lane_id()) - 1ull; }
__device__ __forceinline__ int highest(unsigned long long m) { return 63 - __clzll((long long)m); }
__device__ __forceinline__ uint32_t popc(unsigned long long m) { return (uint32_t)__popcll(m); }

// exclusive prefix sum over the 64 lanes; total = sum of all lanes.  DPP row shifts inside the
// rows of 16 lanes, then the two row broadcasts (lane 15 -> next row, lane 31 -> upper half):
// six adds, no LDS traffic (a __shfl_up ladder is six ds_bpermute round trips).
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t &total) {
  uint32_t x = v;
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1, 3
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2, 3
  total = (uint32_t)__builtin_amdgcn_readlane((int)x, WAVE - 1);
  return x - v;
}

// inclusive prefix sum of a 64-bit value over the 64 lanes (lane 63 holds the wave's sum): the scan kernels' row
// offsets, a few calls per wave -- a shuffle ladder, the DPP forms move 32 bits
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v) {
  const uint32_t lane = lane_id();
  uint64_t x = v;
#pragma unroll
  for (uint32_t o = 1; o < WAVE; o <<= 1) {
    const uint64_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  return x;
}

// minimum / maximum over the 64 lanes, the same DPP ladder: a lane without a source keeps its own value (`old` is the
// value itself), lane 63 ends up with the result.
#define DTK_WAVE_FOLD(x, op)                                                                   \
  do {                                                                                         \
    x = op(x, __builtin_amdgcn_update_dpp(x, x, 0x111, 0xF, 0xF, false)); /* row_shr:1 */      \
    x = op(x, __builtin_amdgcn_update_dpp(x, x, 0x112, 0xF, 0xF, false)); /* row_shr:2 */      \
    x = op(x, __builtin_amdgcn_update_dpp(x, x, 0x114, 0xF, 0xF, false)); /* row_shr:4 */      \
    x = op(x, __builtin_amdgcn_update_dpp(x, x, 0x118, 0xF, 0xF, false)); /* row_shr:8 */      \
    x = op(x, __builtin_amdgcn_update_dpp(x, x, 0x142, 0xA, 0xF, false)); /* row_bcast:15 */   \
    x = op(x, __builtin_amdgcn_update_dpp(x, x, 0x143, 0xC, 0xF, false)); /* row_bcast:31 */   \
  } while (0)
__device__ __forceinline__ int32_t wave_min(int32_t v) {
  int x = v;
  DTK_WAVE_FOLD(x, min);
  return __builtin_amdgcn_readlane(x, WAVE - 1);
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
  int x = v;
  DTK_WAVE_FOLD(x, max);
  return __builtin_amdgcn_readlane(x, WAVE - 1);
}

// sum over the 64 lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// exclusive prefix sum of a 32-bit value over the block's 256 threads (four waves: wave_excl_scan, the wave totals
// through LDS); wave_tot: 256 / WAVE words of LDS
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wave_tot, uint32_t &total) {
  uint32_t wt;
  const uint32_t x = wave_excl_scan(v, wt);
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous use of wave_tot has been read)
  if (lane_id() == 0u) wave_tot[wave] = wt;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < 256u / WAVE; k++) {
    const uint32_t t = wave_tot[k];
    before += k < wave ? t : 0u;
    total += t;
  }
  return before + x;
}

// exclusive prefix sum of a 64-bit value over the block's 256 threads; wave_tot: 256 / WAVE words of LDS
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, uint64_t *wave_tot, uint64_t &total) {
  const uint64_t inc = wave_incl_scan64(v);
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous use of wave_tot has been read)
  if (lane_id() == WAVE - 1u) wave_tot[wave] = inc;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < 256u / WAVE; k++) {
    const uint64_t t = wave_tot[k];
    before += k < wave ? t : 0u;
    total += t;
  }
  return before + inc - v;
}

// exclusive scan of base[0 .. n) in place by one block of 256 threads, in rounds of 256 consecutive entries with a
// carry; returns the sum.  T: 32 or 64 bits, the width of the block scan
template <class T>
__device__ __forceinline__ T scan_row_in_place(T *base, uint32_t n, T *wave_tot) {
  T carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 256u) {  // (block-uniform trip count)
    const uint32_t i = i0 + threadIdx.x;
    const T v = i < n ? base[i] : 0u;
    T total, x;
    if constexpr (sizeof(T) == 8) x = block_excl_scan64(v, wave_tot, total); else x = block_excl_scan(v, wave_tot, total);
    if (i < n) base[i] = carry + x;
    carry += total;
  }
  return carry;
}
__device__ __forceinline__ uint64_t scan_row64(uint64_t *base, uint32_t n, uint64_t *wave_tot) {
  return scan_row_in_place(base, n, wave_tot);
}
__device__ __forceinline__ uint32_t scan_row(uint32_t *base, uint32_t n, uint32_t *wave_tot) {
  return scan_row_in_place(base, n, wave_tot);
}

// first i in [lo, hi) for which pred(i) is false, else hi; pred is monotone: true on a prefix of the range, false behind
template <class I, class P>
__device__ __forceinline__ I first_false(I lo, I hi, P pred) {
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    if (pred(mid)) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// first i in [0, n) with a[i] >= x, else n
__device__ __forceinline__ uint32_t lower_bound32(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// the length of the slice's event list, or 0xFFFFFFFF if it did not fit its arrays (nothing is computed then)
template <class A>
__device__ __forceinline__ uint32_t evl_entries(const A &a) {
  const uint32_t n = *a.evl_count;
  return n > a.evl_cap ? 0xFFFFFFFFu : n;
}

// ---- the U+FFFD rule of the renderers (dtk_render.hip, dtk_streamrender.hip): string(buf[offset:]) re-encodes the
// window's runes (token_writer.go:85), so a byte that did not decode leaves as EF BF BD.  Such bytes are the rune starts
// of width 1 whose rune is >= 256 in the symbol stream.
__device__ __forceinline__ bool sym_invalid_byte(const DtkSym &S, uint64_t i) {
  const uint32_t e = dtk_sym_entry(S, i);
  return DTK_SYM_WIDTH(e) == 1u && ((e >> DTK_SYM_CLS_SHIFT) & 3u) >= 2u;
}

// how many of the text's bytes [i0, i0 + n) print as U+FFFD: each makes its surface two bytes longer
__device__ __forceinline__ uint32_t sym_invalid_count(const DtkSym &S, uint64_t i0, uint32_t n) {
  uint32_t c = 0;
  for (uint32_t q = 0; q < n; q++) c += sym_invalid_byte(S, i0 + q) ? 1u : 0u;
  return c;
}

// the surface text[i0 .. i0 + n) to out[o ..) with those bytes expanded, nothing stored at or behind `cap`: a
// replacement only if its three bytes fit, a plain byte only if it fits; the offset advances either way
__device__ __forceinline__ void sym_expand(const DtkSym &S, const uint8_t *__restrict__ text, uint64_t i0, uint32_t n,
                                           uint8_t *__restrict__ out, uint64_t o, uint64_t cap) {
  for (uint32_t q = 0; q < n; q++) {
    if (sym_invalid_byte(S, i0 + q)) {
      if (o + 3u <= cap) { out[o] = 0xEF; out[o + 1] = 0xBF; out[o + 2] = 0xBD; }
      o += 3u;
    } else {
      if (o < cap) out[o] = text[i0 + q];
      o += 1u;
    }
  }
}

// 64-bit words that hold n 32-bit ones (a workspace is laid out in 64-bit words)
inline uint64_t words32(uint64_t n) { return (n + 1u) / 2u; }

__device__ __forceinline__ uint32_t doc_of(const uint64_t *__restrict__ doc_off, uint32_t lo, uint32_t hi,
                                           uint64_t g) {
  // largest d in [lo, hi) with doc_off[d] <= g   (invariant: doc_off[lo] <= g < doc_off[hi])
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (doc_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One thread per document: nothing to do unless a lane failed; then the lane
// `bad` started from a true state (every lane before it checked out), so where it
// really ended is the true record of its successor: redo from `bad` on.
__device__ __forceinline__ void mark_redo(const DtkSpecArgs &S, uint32_t d, uint32_t bad, uint32_t *redo_out,
                                          uint32_t *n_bad) {
  const uint32_t L0 = S.chunk_off[d], L1 = S.chunk_off[d + 1];
  DtkLaneState en = S.lane_end[bad];
  en.flags &= (LANE_F_SENT | LANE_F_TEXT | LANE_F_OK);
  if (en.p != 0xFFFFFFFFu && bad + 1 < L1) S.lane_start[bad + 1] = en;
  // (ran to EOF: no later lane has a sync point -- k_redo_spread withdraws their records)
  // The round walks again from the last lane before `bad` that owns anything: it started from a true record as
  // well, and everything a lane behind the broken link can have reported lies behind that record -- the round
  // clears from there on without having to tell true reports from false ones.
  uint32_t r0 = bad;
  if (bad > L0) {
    r0 = bad - 1u;
    while (r0 > L0 && S.lane_end[r0].p == S.lane_start[r0].p) r0--;
  }
  redo_out[d] = r0;
  atomicAdd(n_bad, 1u);
}

