// dtk_render.hip -- NewTokenWriter's byte output on the device (gfx950).
//
// token_writer.go:36-175 restated as a data-parallel gather: what the reference prints call by
// call is, per text,
//     [ surface "\n" per Token (TOKENS) , "\n" per SentenceEnd (SENTENCES) , in call order ]
//     [ token positions  "s e s e ...\n" (TOKEN_POS) ] [ sentence positions (SENTENCE_POS) ]
//     or, without a position flag, one "\n" per TextEnd.
// Every piece has a size that depends only on the compacted arrays, so three exclusive scans
// (surface bytes, token-position digits, sentence-position digits) plus the per-token count of
// earlier SentenceEnd calls give every piece its offset; all separators that are not written
// explicitly are newlines, so the buffer is pre-filled with '\n'.
#include "dtk_device.h"

namespace {

constexpr uint32_t RB = 256;          // threads per block
constexpr uint32_t RI = 4;            // items per thread
constexpr uint32_t RTILE = RB * RI;   // items per block

struct Pair { uint64_t a, p; };

// the text of item k of document d (a token or a sentence int): the first record of the document whose end in `ends`
// lies behind k; text_off[d + 1] for an item behind the last TextEnd (flagged document)
__device__ __forceinline__ uint64_t text_of(const DtkRenderArgs &R, const uint32_t *ends, uint32_t d, uint32_t k) {
  return first_false(R.text_off[d], R.text_off[d + 1], [&](uint64_t g) { return ends[g] <= k; });
}

__device__ __forceinline__ Pair tok_weight(const DtkRenderArgs &R, uint64_t k) {
  Pair w{0, 0};
  if (k < R.n_tok) {
    if (R.flags & 1u) {  // surface + '\n'
      const uint32_t b0 = R.bstart[k], n = R.bend[k] - b0;
      w.a = (uint64_t)n + 1u;
      if (R.sym.base) w.a += 2u * sym_invalid_count(R.sym, R.doc_off[doc_of(R.tok_off, 0u, R.n_docs, k)] + b0, n);
    }
    if (R.flags & 4u) w.p = (uint64_t)dec_len(R.rstart[k]) + dec_len(R.rend[k]) + 2u;  // "s e "
  }
  return w;
}

__device__ __forceinline__ uint64_t sent_weight(const DtkRenderArgs &R, uint64_t s) {
  return (s < R.n_sent && (R.flags & 8u)) ? (uint64_t)dec_len(R.sent[s]) + 1u : 0u;
}

// phase 1: per-tile sums.  grid.x = tiles over tokens, then tiles over sentence ints.
__global__ __launch_bounds__(RB) void k_render_sums(DtkRenderArgs R, uint32_t tok_tiles) {
  __shared__ uint64_t sh[RB / WAVE];
  const uint32_t b = blockIdx.x;
  uint64_t tot;
  if (b < tok_tiles) {
    Pair s{0, 0};
    const uint64_t k0 = (uint64_t)b * RTILE + threadIdx.x * RI;
    for (uint32_t i = 0; i < RI; i++) { const Pair w = tok_weight(R, k0 + i); s.a += w.a; s.p += w.p; }
    (void)block_excl_scan64(s.a, sh, tot);
    if (threadIdx.x == 0) R.blkA[b] = tot;
    (void)block_excl_scan64(s.p, sh, tot);
    if (threadIdx.x == 0) R.blkP[b] = tot;
  } else {
    const uint32_t c = b - tok_tiles;
    uint64_t s = 0;
    const uint64_t s0 = (uint64_t)c * RTILE + threadIdx.x * RI;
    for (uint32_t i = 0; i < RI; i++) s += sent_weight(R, s0 + i);
    (void)block_excl_scan64(s, sh, tot);
    if (threadIdx.x == 0) R.blkQ[c] = tot;
  }
}

// dst[0 .. n) = the exclusive scan of src[0 .. n) by one block of RB threads; returns the sum.  dst may be src, and S
// may be narrower.  Every thread takes a slice of consecutive entries and one block scan links the slices: the rows here
// are long (the bench batch: 2177 tile sums, 4096 documents), and scan_row64's rounds of 256 with a carry, one after the
// other, cost this launch 5 us of the renderer's 145 (profiles/render_shared.txt).
template <class S>
__device__ __forceinline__ uint64_t scan_slices(uint64_t *dst, const S *src, uint32_t n, uint64_t *wave_tot) {
  const uint32_t per = n / RB + (n % RB ? 1u : 0u);
  const uint32_t lo = min(threadIdx.x * per, n), hi = lo + min(per, n - lo);  // ((RB - 1) * per < 2^32)
  uint64_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += src[i];
  uint64_t total;
  uint64_t run = block_excl_scan64(sum, wave_tot, total);
  for (uint32_t i = lo; i < hi; i++) { const uint64_t v = src[i]; dst[i] = run; run += v; }
  return total;
}

// phase 2: exclusive scans of the tile sums and of the per-document SentenceEnd counts (one block):
// ns_off[d] = SentenceEnd calls in documents before d; [n_docs] = all
__global__ __launch_bounds__(RB) void k_render_scan_tiles(DtkRenderArgs R, uint32_t tok_tiles, uint32_t sent_tiles) {
  __shared__ uint64_t sh[RB / WAVE];
  (void)scan_slices(R.blkA, R.blkA, tok_tiles, sh);
  (void)scan_slices(R.blkP, R.blkP, tok_tiles, sh);
  (void)scan_slices(R.blkQ, R.blkQ, sent_tiles, sh);
  const uint64_t all = scan_slices(R.ns_off, R.doc_ns, R.n_docs, sh);
  if (threadIdx.x == 0) R.ns_off[R.n_docs] = all;
}

// phase 3: the scans themselves (A, P over tokens; Q over sentence ints), n+1 entries each
__global__ __launch_bounds__(RB) void k_render_offsets(DtkRenderArgs R, uint32_t tok_tiles) {
  __shared__ uint64_t sh[RB / WAVE];
  const uint32_t b = blockIdx.x;
  uint64_t tot;
  if (b < tok_tiles) {
    Pair w[RI], s{0, 0};
    const uint64_t k0 = (uint64_t)b * RTILE + threadIdx.x * RI;
    for (uint32_t i = 0; i < RI; i++) { w[i] = tok_weight(R, k0 + i); s.a += w[i].a; s.p += w[i].p; }
    uint64_t ra = R.blkA[b] + block_excl_scan64(s.a, sh, tot);
    uint64_t rp = R.blkP[b] + block_excl_scan64(s.p, sh, tot);
    for (uint32_t i = 0; i < RI; i++) {
      if (k0 + i <= R.n_tok) { R.A[k0 + i] = ra; R.P[k0 + i] = rp; }
      ra += w[i].a; rp += w[i].p;
    }
  } else {
    const uint32_t c = b - tok_tiles;
    uint64_t w[RI], s = 0;
    const uint64_t s0 = (uint64_t)c * RTILE + threadIdx.x * RI;
    for (uint32_t i = 0; i < RI; i++) { w[i] = sent_weight(R, s0 + i); s += w[i]; }
    uint64_t rq = R.blkQ[c] + block_excl_scan64(s, sh, tot);
    for (uint32_t i = 0; i < RI; i++) {
      if (s0 + i <= R.n_sent) R.Q[s0 + i] = rq;
      rq += w[i];
    }
  }
}

// per text g (and the sentinel g == n_text): where its three regions start
__global__ __launch_bounds__(RB) void k_render_texts(DtkRenderArgs R) {
  const uint64_t g = (uint64_t)blockIdx.x * RB + threadIdx.x;
  if (g > R.n_text) return;
  const uint64_t S = (R.flags & 2u) ? 1u : 0u;
  const uint64_t NP = (R.flags & 12u) ? 0u : 1u;  // without position flags TextEnd prints "\n"
  if (g == R.n_text) {
    R.tx_base[g] = R.A[R.n_tok] + R.P[R.n_tok] + R.Q[R.n_sent] + S * R.ns_off[R.n_docs] + NP * g;
    return;
  }
  const uint32_t d = doc_of(R.text_off, 0u, R.n_docs, g);
  const bool first = g == R.text_off[d];
  const uint64_t TB = R.tok_off[d] + (first ? 0u : R.ttok[g - 1]), TE = R.tok_off[d] + R.ttok[g];
  const uint64_t QB = R.sent_off[d] + (first ? 0u : R.tsent[g - 1]);
  const uint64_t SS = R.ns_off[d] + (first ? 0u : R.ts_end[g - 1]), SE = R.ns_off[d] + R.ts_end[g];
  const uint64_t base = R.A[TB] + R.P[TB] + R.Q[QB] + S * SS + NP * g;
  const uint64_t pos_start = base + (R.A[TE] - R.A[TB]) + S * (SE - SS);
  const uint64_t sent_start = pos_start + (R.P[TE] - R.P[TB]);
  R.tx_base[g] = base;
  R.tx_stream[g] = base - R.A[TB] - S * SS;  // + A[K] + S * (SentenceEnd calls before token K)
  R.tx_pos[g] = pos_start - R.P[TB];         // + P[K]
  R.tx_sent[g] = sent_start - R.Q[QB];       // + Q[s]
}

__global__ __launch_bounds__(RB) void k_render_doc_offsets(DtkRenderArgs R) {
  const uint64_t d = (uint64_t)blockIdx.x * RB + threadIdx.x;
  if (d > R.n_docs) return;
  R.out_off[d] = R.tx_base[d == R.n_docs ? R.n_text : R.text_off[d]];
}

// one thread per token: surface bytes and/or its two position ints
__global__ __launch_bounds__(RB) void k_render_tokens(DtkRenderArgs R) {
  const uint64_t K = (uint64_t)blockIdx.x * RB + threadIdx.x;
  if (K >= R.n_tok) return;
  const uint32_t d = doc_of(R.tok_off, 0u, R.n_docs, K);
  const uint32_t k = (uint32_t)(K - R.tok_off[d]);
  const uint64_t g = text_of(R, R.ttok, d, k);
  if (g >= R.text_off[d + 1]) return;
  if (R.flags & 1u) {
    const uint64_t S = (R.flags & 2u) ? 1u : 0u;
    const uint64_t o = R.tx_stream[g] + R.A[K] + S * (R.ns_off[d] + R.sbefore[K]);
    const uint32_t b0 = R.bstart[K], n = R.bend[K] - b0;
    if (o + n <= R.out_total) {
      const uint64_t i0 = R.doc_off[d] + b0;
      if (!R.sym.base) {
        for (uint32_t i = 0; i < n; i++) R.out[o + i] = R.text[i0 + i];
      } else {  // the batch has bytes that print as U+FFFD
        sym_expand(R.sym, R.text, i0, n, R.out, o, R.out_total);
      }
    }
  }
  if (R.flags & 4u) {
    uint64_t o = R.tx_pos[g] + R.P[K];
    const int32_t rs = R.rstart[K], re = R.rend[K];
    const uint32_t n1 = dec_len(rs), n2 = dec_len(re);
    if (o + n1 + n2 + 2u <= R.out_total) {
      dec_put(R.out + o, rs, n1);
      R.out[o + n1] = ' ';
      dec_put(R.out + o + n1 + 1u, re, n2);
      if (k + 1u != R.ttok[g]) R.out[o + n1 + 1u + n2] = ' ';  // the line's last int keeps the '\n'
    }
  }
}

// one thread per sentence int (SENTENCE_POS)
__global__ __launch_bounds__(RB) void k_render_sents(DtkRenderArgs R) {
  const uint64_t s = (uint64_t)blockIdx.x * RB + threadIdx.x;
  if (s >= R.n_sent) return;
  const uint32_t d = doc_of(R.sent_off, 0u, R.n_docs, s);
  const uint32_t i = (uint32_t)(s - R.sent_off[d]);
  const uint64_t g = text_of(R, R.tsent, d, i);
  if (g >= R.text_off[d + 1]) return;
  const uint64_t o = R.tx_sent[g] + R.Q[s];
  const int32_t v = R.sent[s];
  const uint32_t n = dec_len(v);
  if (o + n + 1u <= R.out_total) {
    dec_put(R.out + o, v, n);
    if (i + 1u != R.tsent[g]) R.out[o + n] = ' ';
  }
}

}  // namespace

static inline uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + 1 + RTILE - 1) / RTILE); }  // n+1 entries

extern "C" uint32_t dtk_render_tiles(uint64_t n) { return tiles_of(n); }

// Lays the workspace out in `ws` (64-bit words; null: only the size is wanted) and returns its words.
extern "C" uint64_t dtk_render_ws(DtkRenderArgs *R, uint64_t *ws) {
  const uint64_t nt = R->n_tok, ns = R->n_sent, nx = R->n_text, tt = tiles_of(nt), st = tiles_of(ns);
  uint64_t at = 0;
  auto take = [&](uint64_t words) { uint64_t *p = ws ? ws + at : nullptr; at += words; return p; };
  R->A = take(nt + 1u); R->P = take(nt + 1u); R->Q = take(ns + 1u);
  R->blkA = take(tt); R->blkP = take(tt); R->blkQ = take(st);
  R->ns_off = take((uint64_t)R->n_docs + 1u);
  R->tx_base = take(nx + 1u); R->tx_stream = take(nx + 1u); R->tx_pos = take(nx + 1u); R->tx_sent = take(nx + 1u);
  return at + 8u;  // (eight spare words, as ever)
}

// stage 0: sizes (sums, scans, per-text regions, per-document offsets); stage 1: bytes
extern "C" int dtk_launch_render(const DtkRenderArgs *R, int stage, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  const uint32_t tt = tiles_of(R->n_tok), st = tiles_of(R->n_sent);
  if (stage == 0) {
    hipLaunchKernelGGL(k_render_sums, dim3(tt + st), dim3(RB), 0, s, *R, tt);
    hipLaunchKernelGGL(k_render_scan_tiles, dim3(1), dim3(RB), 0, s, *R, tt, st);
    hipLaunchKernelGGL(k_render_offsets, dim3(tt + st), dim3(RB), 0, s, *R, tt);
    hipLaunchKernelGGL(k_render_texts, dim3((uint32_t)((R->n_text + 1 + RB - 1) / RB)), dim3(RB), 0, s, *R);
    hipLaunchKernelGGL(k_render_doc_offsets, dim3((R->n_docs + 1 + RB - 1) / RB), dim3(RB), 0, s, *R);
  } else {
    if (R->n_tok && (R->flags & 5u))
      hipLaunchKernelGGL(k_render_tokens, dim3((uint32_t)((R->n_tok + RB - 1) / RB)), dim3(RB), 0, s, *R);
    if (R->n_sent && (R->flags & 8u))
      hipLaunchKernelGGL(k_render_sents, dim3((uint32_t)((R->n_sent + RB - 1) / RB)), dim3(RB), 0, s, *R);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
