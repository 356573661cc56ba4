// dtk_evlist.hip -- DTK_R_EVENT_LIST (include/datok_gpu.h): the sparse events of a closure replay as a list.
//
// Of the five event bitmaps a replay needs END and START only as tok_bend / tok_bstart; the other three (SEPS, TEOT,
// SEOT) hold about one set bit per sentence and still cost three bits per input byte on the link.  This unit compacts
// their union  u = SEPS | TEOT | SEOT  into rows {position, kinds} with a CSR over documents.  It runs as four plain
// launches on the download stream, in front of the copies (where k_pack_r16 and k_pack_blk run): no block waits for
// another block, the order between the steps is the stream's.
//
//   k_evl_count   a block takes a tile of EVL_TILE_WORDS consecutive words: its threads load their words of the three
//                 bitmaps, the popcounts of u are summed over the block, one count per tile
//   k_evl_scan    one block scans the tile counts into tile bases (in place), writes the total to evl_off[n_docs] and
//                 to the count word the host reads behind the copies
//   k_evl_write   the same tiling: a block scan gives every thread its first row; the thread walks the set bits of its
//                 words.  The document of global bit g is the last d with doc_off[d] + d <= g: found once per thread by
//                 binary search, then advanced linearly (consecutive bits mostly stay in one document)
//   k_evl_rows    one thread per document: evl_off[d] = lower bound of doc_off[d] + d in the rows' global bits --
//                 documents without entries, runs of empty documents and both ends of the batch come out by construction
//
// Bits at or behind n_bits = doc_off[n_docs] + n_docs are masked off in both passes (nothing promises a clean slack in
// the last word).  k_evl_write and k_evl_rows return at once when the total exceeds `cap`, and write no row at or
// behind it.
#include <algorithm>

#include "dtk_device.h"

namespace {

constexpr uint32_t EVL_THREADS = 256;
constexpr uint32_t EVL_WORDS = 4;  // per thread: one 16-byte load of each bitmap
constexpr uint32_t EVL_TILE_WORDS = EVL_THREADS * EVL_WORDS;  // 32 768 cursor positions per block

struct EvlWords { uint32_t seps[EVL_WORDS], teot[EVL_WORDS], seot[EVL_WORDS]; };

// The thread's words of the three bitmaps, bits at or behind n_bits cleared.  Bitmap k starts at word k * bit_words: a
// 16-byte load only where that address allows it (wide == both the base and bit_words are multiples of 16 bytes).
__device__ __forceinline__ void evl_load(const DtkEvListArgs &A, uint32_t w0, bool wide, EvlWords &W) {
  const uint32_t *seps = A.bits + (uint64_t)EVB_SEPS * A.bit_words, *teot = A.bits + (uint64_t)EVB_TEOT * A.bit_words,
                 *seot = A.bits + (uint64_t)EVB_SEOT * A.bit_words;
  if (wide && w0 + EVL_WORDS <= A.bit_words) {
    const uint4 a = *reinterpret_cast<const uint4 *>(seps + w0), b = *reinterpret_cast<const uint4 *>(teot + w0),
                c = *reinterpret_cast<const uint4 *>(seot + w0);
    W.seps[0] = a.x; W.seps[1] = a.y; W.seps[2] = a.z; W.seps[3] = a.w;
    W.teot[0] = b.x; W.teot[1] = b.y; W.teot[2] = b.z; W.teot[3] = b.w;
    W.seot[0] = c.x; W.seot[1] = c.y; W.seot[2] = c.z; W.seot[3] = c.w;
  } else {
#pragma unroll
    for (uint32_t i = 0; i < EVL_WORDS; i++) {
      const bool in = w0 + i < A.bit_words;
      W.seps[i] = in ? seps[w0 + i] : 0u; W.teot[i] = in ? teot[w0 + i] : 0u; W.seot[i] = in ? seot[w0 + i] : 0u;
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < EVL_WORDS; i++) {
    const uint64_t g0 = (uint64_t)(w0 + i) << 5;
    const uint32_t keep = g0 >= A.n_bits ? 0u : (A.n_bits - g0 >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)(A.n_bits - g0)) - 1u);
    W.seps[i] &= keep; W.teot[i] &= keep; W.seot[i] &= keep;
  }
}

__device__ __forceinline__ uint32_t evl_popc(const EvlWords &W) {
  uint32_t c = 0;
#pragma unroll
  for (uint32_t i = 0; i < EVL_WORDS; i++) c += (uint32_t)__popc(W.seps[i] | W.teot[i] | W.seot[i]);
  return c;
}

__device__ __forceinline__ bool evl_wide(const DtkEvListArgs &A) {
  return ((uintptr_t)A.bits & 15u) == 0u && (A.bit_words & 3u) == 0u;
}

__global__ __launch_bounds__(256) void k_evl_count(DtkEvListArgs A) {
  __shared__ uint32_t wave_tot[EVL_THREADS / WAVE];
  EvlWords W;
  evl_load(A, blockIdx.x * EVL_TILE_WORDS + threadIdx.x * EVL_WORDS, evl_wide(A), W);
  uint32_t total;
  (void)block_excl_scan(evl_popc(W), wave_tot, total);
  if (threadIdx.x == 0u) A.tile_base[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_evl_scan(DtkEvListArgs A) {
  __shared__ uint32_t wave_tot[EVL_THREADS / WAVE];
  const uint32_t all = scan_row(A.tile_base, A.n_tiles, wave_tot);
  if (threadIdx.x == 0u) { A.evl_off[A.n_docs] = all; *A.count = all; }
}

__global__ __launch_bounds__(256) void k_evl_write(DtkEvListArgs A) {
  __shared__ uint32_t wave_tot[EVL_THREADS / WAVE];
  const uint32_t n = *A.count;
  if (n > A.cap) return;  // (block-uniform) the host grows the arrays and launches again
  EvlWords W;
  const uint32_t w0 = blockIdx.x * EVL_TILE_WORDS + threadIdx.x * EVL_WORDS;
  evl_load(A, w0, evl_wide(A), W);
  const uint32_t c = evl_popc(W);
  uint32_t total;
  uint32_t row = A.tile_base[blockIdx.x] + block_excl_scan(c, wave_tot, total);
  if (c == 0u) return;
  uint32_t d = 0xFFFFFFFFu;
  uint64_t d_bit0 = 0, next_bit0 = 0;  // bit of position 0 of document d / d + 1 (the batch's end behind the last)
#pragma unroll
  for (uint32_t i = 0; i < EVL_WORDS; i++) {
    uint32_t u = W.seps[i] | W.teot[i] | W.seot[i];
    while (u) {
      const uint32_t bit = (uint32_t)__builtin_ctz(u);
      u &= u - 1u;
      const uint64_t g = ((uint64_t)(w0 + i) << 5) + bit;  // (< n_bits: evl_load masked the rest)
      if (d == 0xFFFFFFFFu) {
        // the last d in [0, n_docs) with doc_off[d] + d <= g   (doc_off[0] + 0 = 0 <= g)
        uint32_t lo = 0, hi = A.n_docs;
        while (hi - lo > 1u) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (A.doc_off[mid] + mid <= g) lo = mid; else hi = mid;
        }
        d = lo;
        d_bit0 = A.doc_off[d] + d;
        next_bit0 = A.doc_off[d + 1] + d + 1u;
      }
      while (g >= next_bit0 && d + 1u < A.n_docs) {
        d++;
        d_bit0 = next_bit0;
        next_bit0 = A.doc_off[d + 1] + d + 1u;
      }
      if (row < A.cap) {
        A.evl_pos[row] = (uint32_t)(g - d_bit0);
        A.evl_kind[row] = (uint8_t)(((W.seot[i] >> bit) & 1u) * DTK_EVL_K_SEOT | ((W.teot[i] >> bit) & 1u) * DTK_EVL_K_TEOT |
                                    ((W.seps[i] >> bit) & 1u) * DTK_EVL_K_SEPS);
        A.evl_bit[row] = (uint32_t)g;
      }
      row++;
    }
  }
}

__global__ __launch_bounds__(256) void k_evl_rows(DtkEvListArgs A) {
  const uint32_t n = *A.count;
  if (n > A.cap) return;
  const uint32_t d = blockIdx.x * EVL_THREADS + threadIdx.x;
  if (d >= A.n_docs) return;
  const uint64_t key = A.doc_off[d] + d;
  // the first row in [0, n) whose bit is >= key, or n
  A.evl_off[d] = first_false(0u, n, [&](uint32_t r) { return (uint64_t)A.evl_bit[r] < key; });
}

}  // namespace

extern "C" uint32_t dtk_evlist_tiles(uint64_t n_bits, uint32_t bit_words) {
  const uint64_t words = (n_bits + 31u) / 32u;
  return (uint32_t)((std::min<uint64_t>(words, bit_words) + EVL_TILE_WORDS - 1u) / EVL_TILE_WORDS);
}

extern "C" int dtk_launch_evlist(const DtkEvListArgs *args, void *stream) {
  DtkEvListArgs A = *args;
  hipStream_t s = (hipStream_t)stream;
  if (A.n_docs == 0 || A.n_bits > 0xFFFFFFFFull || A.n_tiles != dtk_evlist_tiles(A.n_bits, A.bit_words)) return 1;
  if (A.n_tiles) hipLaunchKernelGGL(k_evl_count, dim3(A.n_tiles), dim3(EVL_THREADS), 0, s, A);
  hipLaunchKernelGGL(k_evl_scan, dim3(1), dim3(EVL_THREADS), 0, s, A);
  if (A.n_tiles) hipLaunchKernelGGL(k_evl_write, dim3(A.n_tiles), dim3(EVL_THREADS), 0, s, A);
  hipLaunchKernelGGL(k_evl_rows, dim3((A.n_docs + EVL_THREADS - 1u) / EVL_THREADS), dim3(EVL_THREADS), 0, s, A);
  return (int)hipGetLastError();
}
