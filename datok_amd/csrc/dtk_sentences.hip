// dtk_sentences.hip -- DTK_R_SENTENCES (include/datok_gpu.h): a batch's sentences as rows.
//
// A sentence is a maximal non-empty run of Token calls with no SentenceEnd / TextEnd between them.  Over the event
// bitmaps that is a one-bit machine per document: f = 1 at the document's bit 0, then per cursor in ascending order
//   SEOT or TEOT: f = 1;   END: the token is a sentence's first iff f, then f = 0;   SEPS: f = 1.
// A document start is an event like SEOT (it sets f in front of the cursor's END), so the machine runs over the
// whole bit space of the batch at once.  In one 32-bit word, with R = starts | SEOT | TEOT, E = END, S = SEPS, the
// state behind a cursor is 1 where A = S | (R & ~E) has a bit, 0 where B = E & ~S has one, else the state in front of
// it: the carry chain of the addition ~B + A, so   in = (~B + A + carry_in) ^ ~B ^ A   holds the state in front of
// every cursor of the word and the sum's bit 32 the state behind it; first = E & (R | in).
//
// Plain launches on the download stream, in front of the copies (where k_evl_* run); no block waits for another:
//   k_sen_count   a block takes a tile of SEN_TILE_WORDS words; a thread its 4 words of each bitmap (16-byte loads)
//                 and the document starts among its 128 cursors.  Per tile: the sentence-first tokens if f comes in
//                 as 0, whether one more comes with f = 1 (only the tile's first END can depend on it), and the state
//                 behind the tile (pass-through for a tile without an event)
//   k_sen_scan    one block resolves every tile's incoming f and row base (in place), writes the total to
//                 sen_off[n_docs] and to the count word the host reads
//   k_sen_write   the same tiling with f known: per sentence-first END bit the bit, its document, and the token's
//                 index in the document (the cursor's place in the document's tok_bend row, by binary search)
//   k_sen_rows    one thread per document: sen_off[d] by lower bound on the rows' bits, and the document's
//                 text_sen_end rows by lower bound on its rows' first tokens
//   k_sen_gather  one thread per row: sen_tok_end and the spans, gathered from the token rows
//
// Bits at or behind n_bits = doc_off[n_docs] + n_docs are masked off.  When the total exceeds `cap` the last three
// kernels return at once and no row is written; k_sen_scan has written the total to the count word and to
// sen_off[n_docs], which say so.
#include <algorithm>

#include "dtk_device.h"

namespace {

constexpr uint32_t SEN_THREADS = 256;
constexpr uint32_t SEN_WORDS = 4;  // per thread: one 16-byte load of each bitmap
constexpr uint32_t SEN_TILE_WORDS = SEN_THREADS * SEN_WORDS;  // 32 768 cursor positions per block

// a thread's or a tile's effect on f: 0 = none (pass-through), 2 = leaves f = 0, 3 = leaves f = 1
constexpr uint32_t T_SET = 2u;

struct SenWords { uint32_t r[SEN_WORDS], e[SEN_WORDS], s[SEN_WORDS]; };  // R (without the starts yet), E, S

__device__ __forceinline__ bool sen_wide(const DtkSentencesArgs &A) {
  return ((uintptr_t)A.bits & 15u) == 0u && (A.bit_words & 3u) == 0u;
}

// the first d in [0, n_docs) whose bit 0 is at or behind g, else n_docs
__device__ __forceinline__ uint32_t first_doc_from(const DtkSentencesArgs &A, uint64_t g) {
  return first_false(0u, A.n_docs, [&](uint32_t d) { return A.doc_off[d] + d < g; });
}

// The thread's words, bits at or behind n_bits cleared, the document starts among them ORed into R.  Returns the
// first document that starts at or behind the thread's first cursor (n_docs: none).
__device__ __forceinline__ uint32_t sen_load(const DtkSentencesArgs &A, uint32_t w0, bool wide, SenWords &W) {
  const uint32_t *end = A.bits + (uint64_t)EVB_END * A.bit_words, *seps = A.bits + (uint64_t)EVB_SEPS * A.bit_words,
                 *teot = A.bits + (uint64_t)EVB_TEOT * A.bit_words, *seot = A.bits + (uint64_t)EVB_SEOT * A.bit_words;
  if (wide && w0 + SEN_WORDS <= A.bit_words) {
    const uint4 a = *reinterpret_cast<const uint4 *>(end + w0), b = *reinterpret_cast<const uint4 *>(seps + w0),
                c = *reinterpret_cast<const uint4 *>(teot + w0), d = *reinterpret_cast<const uint4 *>(seot + w0);
    W.e[0] = a.x; W.e[1] = a.y; W.e[2] = a.z; W.e[3] = a.w;
    W.s[0] = b.x; W.s[1] = b.y; W.s[2] = b.z; W.s[3] = b.w;
    W.r[0] = c.x | d.x; W.r[1] = c.y | d.y; W.r[2] = c.z | d.z; W.r[3] = c.w | d.w;
  } else {
#pragma unroll
    for (uint32_t i = 0; i < SEN_WORDS; i++) {
      const bool in = w0 + i < A.bit_words;
      W.e[i] = in ? end[w0 + i] : 0u; W.s[i] = in ? seps[w0 + i] : 0u;
      W.r[i] = in ? (teot[w0 + i] | seot[w0 + i]) : 0u;
    }
  }
  const uint64_t g0 = (uint64_t)w0 << 5;
#pragma unroll
  for (uint32_t i = 0; i < SEN_WORDS; i++) {
    const uint64_t g = g0 + 32u * i;
    const uint32_t keep = g >= A.n_bits ? 0u : (A.n_bits - g >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)(A.n_bits - g)) - 1u);
    W.e[i] &= keep; W.s[i] &= keep; W.r[i] &= keep;
  }
  if (g0 >= A.n_bits) return A.n_docs;
  const uint32_t d0 = first_doc_from(A, g0);
  for (uint32_t d = d0; d < A.n_docs; d++) {  // (a run of empty documents puts one start on every bit)
    const uint64_t rel = A.doc_off[d] + d - g0;
    if (rel >= 32u * SEN_WORDS) break;
#pragma unroll
    for (uint32_t i = 0; i < SEN_WORDS; i++)
      if ((uint32_t)rel >> 5 == i) W.r[i] |= 1u << ((uint32_t)rel & 31u);
  }
  return d0;
}

// The machine over the thread's words from f = cin: the sentence-first END bits, their number, and f behind them.
__device__ __forceinline__ uint32_t sen_chain(const SenWords &W, uint32_t cin, uint32_t first[SEN_WORDS], uint32_t &cout) {
  uint32_t n = 0, c = cin;
#pragma unroll
  for (uint32_t i = 0; i < SEN_WORDS; i++) {
    const uint32_t a = W.s[i] | (W.r[i] & ~W.e[i]), nb = ~(W.e[i] & ~W.s[i]);
    const uint64_t sum = (uint64_t)nb + a + c;
    const uint32_t in = (uint32_t)sum ^ nb ^ a;
    c = (uint32_t)(sum >> 32);
    first[i] = W.e[i] & (W.r[i] | in);
    n += (uint32_t)__popc(first[i]);
  }
  cout = c;
  return n;
}

__device__ __forceinline__ bool sen_any(const SenWords &W) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t i = 0; i < SEN_WORDS; i++) m |= W.r[i] | W.e[i] | W.s[i];
  return m != 0u;
}

// f in front of every thread of the block from the threads' effects t and the block's incoming f.  from_in: no
// thread in front of this one has an effect, the value is block_in itself.  block_t: the block's own effect.
// wave_t: SEN_THREADS / WAVE words of LDS.
__device__ __forceinline__ uint32_t sen_resolve(uint32_t t, uint32_t block_in, uint32_t *wave_t, bool &from_in, uint32_t &block_t) {
  const unsigned long long set = __ballot((t & T_SET) != 0u), one = __ballot(t == (T_SET | 1u));
  const unsigned long long prev = set & lanemask_lt();
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous use of wave_t has been read)
  if (lane_id() == 0u) wave_t[wave] = set ? (T_SET | (uint32_t)((one >> highest(set)) & 1ull)) : 0u;
  __syncthreads();
  uint32_t in = block_in;
  bool fin = true;
  block_t = 0u;
#pragma unroll
  for (uint32_t k = 0; k < SEN_THREADS / WAVE; k++) {
    const uint32_t w = wave_t[k];
    if (w & T_SET) {
      if (k < wave) { in = w & 1u; fin = false; }
      block_t = w;
    }
  }
  if (prev) { in = (uint32_t)((one >> highest(prev)) & 1ull); fin = false; }
  from_in = fin;
  return in;
}

// a tile's summary word: its count with f = 0 coming in | one more with f = 1 << 24 | its effect << 28
constexpr uint32_t SUM_CNT = 0xFFFFFu, SUM_DEP_SHIFT = 24, SUM_T_SHIFT = 28;

__global__ __launch_bounds__(256) void k_sen_count(DtkSentencesArgs A) {
  __shared__ uint32_t wave_t[SEN_THREADS / WAVE], wave_tot[SEN_THREADS / WAVE];
  SenWords W;
  (void)sen_load(A, blockIdx.x * SEN_TILE_WORDS + threadIdx.x * SEN_WORDS, sen_wide(A), W);
  uint32_t first[SEN_WORDS], c0, c1;
  const uint32_t n0 = sen_chain(W, 0u, first, c0), n1 = sen_chain(W, 1u, first, c1);
  const uint32_t t = sen_any(W) ? (T_SET | c0) : 0u;
  bool from_in;
  uint32_t tile_t;
  const uint32_t in = sen_resolve(t, 0u, wave_t, from_in, tile_t);
  // (only the tile's first thread with an effect can count differently for the two incoming states: at most one)
  const uint32_t v = (in ? n1 : n0) | ((from_in && n1 != n0) ? 1u << SUM_DEP_SHIFT : 0u);
  uint32_t total;
  (void)block_excl_scan(v, wave_tot, total);
  if (threadIdx.x == 0u) A.tile_base[blockIdx.x] = total | tile_t << SUM_T_SHIFT;
}

__global__ __launch_bounds__(256) void k_sen_scan(DtkSentencesArgs A) {
  __shared__ uint32_t wave_t[SEN_THREADS / WAVE], wave_tot[SEN_THREADS / WAVE];
  uint32_t carry = 0, f = 0;  // (document 0 starts at bit 0: what comes into tile 0 never counts)
  for (uint32_t i0 = 0; i0 < A.n_tiles; i0 += SEN_THREADS) {  // (block-uniform trip count)
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t sum = i < A.n_tiles ? A.tile_base[i] : 0u;
    bool from_in;
    uint32_t chunk_t, total;
    const uint32_t in = sen_resolve(sum >> SUM_T_SHIFT, f, wave_t, from_in, chunk_t);
    const uint32_t v = (sum & SUM_CNT) + (((sum >> SUM_DEP_SHIFT) & 1u) & in);
    const uint32_t x = block_excl_scan(v, wave_tot, total);
    if (i < A.n_tiles) { A.tile_base[i] = carry + x; A.tile_in[i] = in; }
    carry += total;
    if (chunk_t & T_SET) f = chunk_t & 1u;
  }
  if (threadIdx.x == 0u) { A.sen_off[A.n_docs] = carry; *A.count = carry; }
}

__global__ __launch_bounds__(256) void k_sen_write(DtkSentencesArgs A) {
  __shared__ uint32_t wave_t[SEN_THREADS / WAVE], wave_tot[SEN_THREADS / WAVE];
  if (*A.count > A.cap) return;  // (block-uniform) the host grows the arrays and launches again
  SenWords W;
  const uint32_t w0 = blockIdx.x * SEN_TILE_WORDS + threadIdx.x * SEN_WORDS;
  const uint32_t d0 = sen_load(A, w0, sen_wide(A), W);
  uint32_t first[SEN_WORDS], c0;
  (void)sen_chain(W, 0u, first, c0);
  bool from_in;
  uint32_t tile_t;
  const uint32_t in = sen_resolve(sen_any(W) ? (T_SET | c0) : 0u, A.tile_in[blockIdx.x], wave_t, from_in, tile_t);
  const uint32_t c = sen_chain(W, in, first, c0);
  uint32_t total;
  uint32_t row = A.tile_base[blockIdx.x] + block_excl_scan(c, wave_tot, total);
  if (c == 0u) return;
  // the document of the thread's first cursor: the last one that starts at or in front of it (d0 starts at or behind it)
  const uint64_t g0 = (uint64_t)w0 << 5;
  uint32_t d = (d0 < A.n_docs && A.doc_off[d0] + d0 == g0) ? d0 : d0 - 1u;  // (d0 == 0 starts at bit 0 = g0)
  uint64_t d_bit0 = A.doc_off[d] + d, next_bit0 = A.doc_off[d + 1] + d + 1u;
#pragma unroll
  for (uint32_t i = 0; i < SEN_WORDS; i++) {
    uint32_t u = first[i];
    while (u) {
      const uint32_t bit = (uint32_t)__builtin_ctz(u);
      u &= u - 1u;
      const uint64_t g = g0 + 32u * i + bit;  // (< n_bits: sen_load masked the rest)
      while (g >= next_bit0 && d + 1u < A.n_docs) {
        d++;
        d_bit0 = next_bit0;
        next_bit0 = A.doc_off[d + 1] + d + 1u;
      }
      if (row < A.cap) {
        const uint64_t t0 = A.tok_off[d];
        A.sen_bit[row] = (uint32_t)g;
        A.sen_doc[row] = d;
        A.sen_first[row] = lower_bound32(A.tok_bend + t0, (uint32_t)(A.tok_off[d + 1] - t0), (uint32_t)(g - d_bit0));
      }
      row++;
    }
  }
}

__global__ __launch_bounds__(256) void k_sen_rows(DtkSentencesArgs A) {
  const uint32_t n = *A.count;
  if (n > A.cap) return;
  const uint32_t d = blockIdx.x * SEN_THREADS + threadIdx.x;
  if (d >= A.n_docs) return;
  const uint32_t lo = lower_bound32(A.sen_bit, n, (uint32_t)(A.doc_off[d] + d));
  const uint32_t hi = d + 1u < A.n_docs ? lower_bound32(A.sen_bit, n, (uint32_t)(A.doc_off[d + 1] + d + 1u)) : n;
  A.sen_off[d] = lo;
  for (uint64_t g = A.text_off[d]; g < A.text_off[d + 1] && g < A.text_cap; g++)
    A.text_sen_end[g] = lower_bound32(A.sen_first + lo, hi - lo, A.text_tok_end[g]);
}

__global__ __launch_bounds__(256) void k_sen_gather(DtkSentencesArgs A) {
  const uint32_t n = *A.count;
  if (n > A.cap) return;
  const uint32_t i = blockIdx.x * SEN_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = A.sen_doc[i], first = A.sen_first[i];
  const uint64_t t0 = A.tok_off[d];
  const uint32_t cnt = (uint32_t)(A.tok_off[d + 1] - t0);
  const uint32_t end = (i + 1u < n && A.sen_doc[i + 1u] == d) ? A.sen_first[i + 1u] : cnt;
  // (a document with a status bit may have END bits without token rows: such a span reads as 0, nothing is read
  //  outside the document's rows)
  const bool has_first = first < cnt, has_last = end >= 1u && end <= cnt;
  A.sen_tok_end[i] = end;
  A.sen_bstart[i] = has_first ? A.tok_bstart[t0 + first] : 0u;
  A.sen_bend[i] = has_last ? A.tok_bend[t0 + end - 1u] : 0u;
  if (A.tok_rstart) {
    A.sen_rstart[i] = has_first ? A.tok_rstart[t0 + first] : 0;
    A.sen_rend[i] = has_last ? A.tok_rend[t0 + end - 1u] : 0;
  }
}

}  // namespace

extern "C" uint32_t dtk_sentences_tile_bits(void) { return SEN_TILE_WORDS * 32u; }

extern "C" uint32_t dtk_sentences_tiles(uint64_t n_bits, uint32_t bit_words) {
  const uint64_t words = (n_bits + 31u) / 32u;
  return (uint32_t)((std::min<uint64_t>(words, bit_words) + SEN_TILE_WORDS - 1u) / SEN_TILE_WORDS);
}

extern "C" int dtk_launch_sentences(const DtkSentencesArgs *args, void *stream) {
  DtkSentencesArgs A = *args;
  hipStream_t s = (hipStream_t)stream;
  if (A.n_docs == 0 || A.n_bits > 0xFFFFFFFFull || A.n_tiles != dtk_sentences_tiles(A.n_bits, A.bit_words)) return 1;
  if (A.n_tiles) hipLaunchKernelGGL(k_sen_count, dim3(A.n_tiles), dim3(SEN_THREADS), 0, s, A);
  hipLaunchKernelGGL(k_sen_scan, dim3(1), dim3(SEN_THREADS), 0, s, A);
  if (A.n_tiles) hipLaunchKernelGGL(k_sen_write, dim3(A.n_tiles), dim3(SEN_THREADS), 0, s, A);
  hipLaunchKernelGGL(k_sen_rows, dim3((A.n_docs + SEN_THREADS - 1u) / SEN_THREADS), dim3(SEN_THREADS), 0, s, A);
  if (A.cap) hipLaunchKernelGGL(k_sen_gather, dim3((A.cap + SEN_THREADS - 1u) / SEN_THREADS), dim3(SEN_THREADS), 0, s, A);
  return (int)hipGetLastError();
}
