// dtk_streampos_front.h -- the front of the chain that follows a stream writer's state through one slice, shared by the
// units that need a token's 64-bit rune offsets there: dtk_streampos.hip turns them into digits, dtk_streamoffs.hip
// delivers them as arrays.  The calls, the texts ("segments") and the rules are described at the head of
// dtk_streampos.hip.  Here:
//   k_sp_ent_count (twice), k_sp_front_scan 0   SentenceEnd calls and TextEnd entries in front of every entry; te_idx
//   k_sp_tok_runes, k_sp_front_scan 1           v, the text a token belongs to, its SentenceEnd calls; posC in front of a tile
//   sp_tok_positions                            rstart / rend of a tile's tokens (the unit's next kernel calls it)
//   sp_carry_out                                the writer behind the slice's last call
// Everything has internal linkage: a unit that includes this launches its own copies through sp_launch_front.
#pragma once
#include <algorithm>

#include "dtk_device.h"

namespace {

constexpr uint32_t SP_THREADS = 256;
constexpr uint32_t SP_WAVES = SP_THREADS / WAVE;
constexpr uint32_t W_TOKENS = 1u, W_SENTENCES = 2u, W_TOKEN_POS = 4u, W_SENTENCE_POS = 8u, W_NEWLINE = 16u;
constexpr uint64_t SP_NONE = ~0ull;

typedef DtkStreamPosArgs Args;

__device__ __forceinline__ uint32_t sp_bend(const Args &A, uint32_t k) { return std::min(A.tok_bend[k], A.text_len); }

// a sum that starts again at every element with f set: (a then b) = (b.f ? b.s : a.s + b.s, a.f | b.f)
struct Seg { int64_t s; uint32_t f; };
__device__ __forceinline__ Seg seg_join(Seg a, Seg b) {
  Seg r;
  r.s = b.f ? b.s : a.s + b.s;
  r.f = a.f | b.f;
  return r;
}
// inclusive over the block's 256 threads, behind `seed`; total: all 256 without the seed
__device__ __forceinline__ Seg seg_block_incl(Seg x, Seg seed, int64_t *wave_s, uint32_t *wave_f, Seg &total) {
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t o = 1; o < WAVE; o <<= 1) {
    Seg y;
    y.s = (int64_t)__shfl_up((long long)x.s, o);
    y.f = (uint32_t)__shfl_up((int)x.f, o);
    if (lane >= o) x = seg_join(y, x);
  }
  __syncthreads();
  if (lane == WAVE - 1u) { wave_s[wave] = x.s; wave_f[wave] = x.f; }
  __syncthreads();
  Seg before = seed;
  total = Seg{0, 0u};
#pragma unroll
  for (uint32_t k = 0; k < SP_WAVES; k++) {
    const Seg t{wave_s[k], wave_f[k]};
    if (k < wave) before = seg_join(before, t);
    total = seg_join(total, t);
  }
  return seg_join(before, x);
}

// runes that start in [a, z): a byte that does not decode is one
template <bool INV>
__device__ __forceinline__ uint32_t sp_runes(const Args &A, uint32_t a, uint32_t z) {
  uint32_t n = 0;
  for (uint32_t i = a; i < z; i++) n += INV ? (dtk_sym_is_start(A.sym, i) ? 1u : 0u) : ((A.text[i] & 0xC0u) != 0x80u ? 1u : 0u);
  return n;
}

// SentenceEnd calls from entry `ap` on (and `seps` in front of it) up to the next TextEnd or the token `next` (n_tok:
// none), whichever comes first; the tail's SentenceEnd if neither does
__device__ __forceinline__ uint32_t sp_sent_calls(const Args &A, uint32_t E, uint32_t ap, uint32_t seps, uint32_t next) {
  const uint32_t N = (uint32_t)A.n_tok;
  uint32_t b = E;
  bool atb = false;
  if (next < N) {
    const uint32_t bn = sp_bend(A, next);
    b = lower_bound32(A.evl_pos, E, bn);
    atb = b < E && A.evl_pos[b] == bn;
  }
  const uint32_t c0 = (uint32_t)(A.cnt[ap] >> 32);
  const uint32_t tei = c0 < A.hdr->n_te ? A.te_idx[c0] : E;
  const uint32_t stop = std::min(tei, b);
  uint32_t n = (uint32_t)A.cnt[stop] - (uint32_t)A.cnt[ap] + seps;
  // (the entry at `stop` fires in front of the token only if it lies on its cursor or before: its SEOT comes first)
  if (stop < E && (tei < b || atb) && (A.evl_kind[stop] & DTK_EVL_K_SEOT)) n++;
  if (next >= N && tei == E && A.with_tail && (A.doc_tail[0] & DTK_TAIL_S)) n++;
  return n;
}

// ---------------------------------------------------------------- the list's prefix counts
// (second == 0: tile sums only; k_sp_front_scan 0 turns them into what lies in front of a tile)
__global__ __launch_bounds__(256) void k_sp_ent_count(Args A, uint32_t second) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t j = blockIdx.x * SP_THREADS + threadIdx.x;
  uint64_t v = 0;
  if (j < E) {
    const uint32_t kd = A.evl_kind[j];
    v = (uint64_t)(((kd & DTK_EVL_K_SEOT) ? 1u : 0u) + ((kd & DTK_EVL_K_SEPS) ? 1u : 0u)) | ((kd & DTK_EVL_K_TEOT) ? 1ull << 32 : 0ull);
  }
  uint64_t total;
  const uint64_t x = block_excl_scan64(v, wave_tot, total);
  if (second && j < E) A.cnt[j] = A.ent_base[blockIdx.x] + x;
  if (second && j < E && (v >> 32)) A.te_idx[(uint32_t)((A.ent_base[blockIdx.x] + x) >> 32)] = j;
  if (!second && threadIdx.x == 0u) A.ent_base[blockIdx.x] = total;
}

// ---------------------------------------------------------------- tokens: runes and calls
template <bool INV>
__global__ __launch_bounds__(256) void k_sp_tok_runes(Args A) {
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  Seg x{0, 0u};
  if (k < N) {
    const DtkPosCarry c = *A.carry_in;
    const uint32_t be = sp_bend(A, k), bs = std::min(A.tok_bstart[k], be);
    const uint32_t lbk = lower_bound32(A.evl_pos, E, be);
    const uint32_t kd = (lbk < E && A.evl_pos[lbk] == be) ? A.evl_kind[lbk] : 0u;  // the entry on the token's cursor
    const uint32_t te_k = (uint32_t)(A.cnt[lbk] >> 32) + ((kd & DTK_EVL_K_TEOT) ? 1u : 0u);
    uint32_t te_p = 0, between, bp = A.first;
    if (k) {
      bp = sp_bend(A, k - 1u);
      const uint32_t lbp = lower_bound32(A.evl_pos, E, bp);
      const uint32_t kdp = (lbp < E && A.evl_pos[lbp] == bp) ? A.evl_kind[lbp] : 0u;
      te_p = (uint32_t)(A.cnt[lbp] >> 32) + ((kdp & DTK_EVL_K_TEOT) ? 1u : 0u);
      // (an entry on the predecessor's cursor lies between the two with its SEPS only)
      between = (lbk - lbp) - ((kdp && !(kdp & DTK_EVL_K_SEPS)) ? 1u : 0u);
    } else {
      between = lbk;
    }
    between += (kd & (DTK_EVL_K_SEOT | DTK_EVL_K_TEOT)) ? 1u : 0u;
    const bool newseg = te_k != te_p;
    uint32_t B = (A.is_matrix && newseg) ? A.evl_pos[A.te_idx[te_k - 1u]] : bp;
    B = std::min(B, bs);
    const bool sentB = ((A.bits & W_SENTENCE_POS) && between) || (k == 0u && c.sentB);
    const uint32_t off = sp_runes<INV>(A, B, bs), len = sp_runes<INV>(A, bs, be);
    const bool zero = k ? newseg : (!c.init && (newseg || c.posC == 0));  // posC == 0 and not the stream's first token
    const bool fire = (A.bits & W_NEWLINE) && zero && B < A.text_len && A.text[B] == '\n';
    uint32_t n_s = 0;
    if (A.bits & W_SENTENCE_POS)
      n_s = sp_sent_calls(A, E, lbk + (kd ? 1u : 0u), (kd & DTK_EVL_K_SEPS) ? 1u : 0u, k + 1u) & 0x3FFFFFFFu;
    x.s = (int64_t)(off + len) - (fire ? 1 : 0);
    x.f = newseg ? 1u : 0u;
    A.tok_v[k] = (int32_t)x.s;
    A.tok_len[k] = len;
    A.tok_meta[k] = n_s | (newseg ? 1u << 30 : 0u) | (sentB ? 1u << 31 : 0u);
    A.tok_seg[k] = te_k;
  }
  Seg total;
  (void)seg_block_incl(x, Seg{0, 0u}, wave_s, wave_f, total);
  if (threadIdx.x == 0u) { A.tile_sum[blockIdx.x] = total.s; A.tile_flag[blockIdx.x] = total.f; }
}

// ---------------------------------------------------------------- tokens: rstart / rend
// For the block's tile of 256 tokens, behind k_sp_front_scan 1: writes rstart / rend of token k, raises the header's
// flag 1 for a token whose rend is 0 under the newline rule, and returns rend (meta: tok_meta[k], 0 behind the tokens).
__device__ __forceinline__ int64_t sp_tok_positions(const Args &A, uint32_t k, int64_t *wave_s, uint32_t *wave_f, uint32_t &meta) {
  const uint32_t N = (uint32_t)A.n_tok;
  Seg x{0, 0u};
  meta = 0;
  if (k < N) {
    meta = A.tok_meta[k];
    x.s = A.tok_v[k];
    x.f = (meta >> 30) & 1u;
  }
  Seg total;
  const int64_t re = seg_block_incl(x, Seg{A.tile_in[blockIdx.x], 0u}, wave_s, wave_f, total).s;
  if (k < N) {
    A.rstart[k] = re - (int64_t)A.tok_len[k];
    A.rend[k] = re;
    if ((A.bits & W_NEWLINE) && re == 0) atomicOr(&A.hdr->flags, 1u);
  }
  return re;
}

// ---------------------------------------------------------------- the scanning block
// One block, two stages.  A list longer than its arrays: nothing (the unit's last scanning stage tells the host).
__global__ __launch_bounds__(256) void k_sp_front_scan(Args A, uint32_t stage) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  if (stage == 0u) {  // ---- the entries' counts
    const uint64_t sum = scan_row64(A.ent_base, A.ent_tiles, wave_tot);
    if (threadIdx.x != 0u) return;
    A.cnt[E] = sum;
    DtkPosHdr h{};
    h.n_te = (uint32_t)(sum >> 32);
    *A.hdr = h;
    return;
  }
  // ---- stage 1: posC in front of every token tile; the head's SentenceEnd calls
  Seg carry{A.carry_in->posC, 0u};
  for (uint32_t i0 = 0; i0 < A.tok_tiles; i0 += SP_THREADS) {
    const uint32_t i = i0 + threadIdx.x;
    Seg x{0, 0u};
    if (i < A.tok_tiles) { x.s = A.tile_sum[i]; x.f = A.tile_flag[i]; }
    Seg total;
    const Seg inc = seg_block_incl(x, carry, wave_s, wave_f, total);
    // (exclusive: what lies in front of tile i is the inclusive value of tile i - 1)
    const int64_t prev_s = (int64_t)__shfl_up((long long)inc.s, 1u);
    __syncthreads();
    if (lane_id() == WAVE - 1u) wave_s[threadIdx.x >> 6] = inc.s;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    const int64_t before = lane_id() ? prev_s : (wave ? wave_s[wave - 1u] : carry.s);
    if (i < A.tok_tiles) A.tile_in[i] = before;
    carry = seg_join(carry, total);
  }
  if (threadIdx.x != 0u) return;
  const DtkPosCarry c = *A.carry_in;
  if ((A.bits & W_SENTENCE_POS) && c.pos_nonempty) {
    const uint32_t n = sp_sent_calls(A, E, 0u, 0u, 0u);
    A.hdr->head_n = n;
    A.hdr->head_w = (uint64_t)n * (1u + dec_len64(c.posC));
  }
}

// The writer behind the slice's last call.  tf: the first token of the text that is open at the slice's end (text
// n_te); open_sent: that text has a sentence integer of this slice (the head's count for text 0).
__device__ __forceinline__ DtkPosCarry sp_carry_out(const Args &A, const DtkPosCarry &c, uint32_t E, uint32_t tail, uint32_t n_te,
                                                    uint32_t tf, bool open_sent) {
  const uint32_t N = (uint32_t)A.n_tok;
  const bool contp = n_te == 0u && c.pos_nonempty, conts = n_te == 0u && c.sent_nonempty;
  DtkPosCarry o{};
  const bool closed = (tail & DTK_TAIL_E) != 0u;
  o.posC = closed ? 0 : (N > tf ? A.rend[N - 1u] : (n_te ? 0 : c.posC));
  o.pos_nonempty = (!closed && (N > tf || contp)) ? 1u : 0u;
  o.init = (c.init && N == 0u) ? 1u : 0u;
  if (A.bits & W_SENTENCE_POS) {
    uint32_t after = E + tail;  // calls behind the last token
    if (N) {
      const uint32_t be = sp_bend(A, N - 1u);
      const uint32_t lbk = lower_bound32(A.evl_pos, E, be);
      const uint32_t kd = (lbk < E && A.evl_pos[lbk] == be) ? A.evl_kind[lbk] : 0u;
      after = (E - lbk - (kd ? 1u : 0u)) + ((kd & DTK_EVL_K_SEPS) ? 1u : 0u) + tail;
    }
    o.sentB = (N ? after != 0u : (c.sentB || after != 0u)) ? 1u : 0u;
    o.sent_nonempty = (!closed && (open_sent || conts)) ? 1u : 0u;
  } else {  // (token_writer.go:60-63 runs in every position mode; nothing sets sentB again or clears sent)
    o.sentB = (c.sentB && N == 0u) ? 1u : 0u;
    o.sent_nonempty = (c.sent_nonempty || (c.sentB && N)) ? 1u : 0u;
  }
  return o;
}

// the five launches in front of a unit's own kernels; mark() is called behind each (a measurement's events)
template <class Mark>
inline void sp_launch_front(const Args &A, hipStream_t s, Mark &&mark) {
  const bool inv = A.sym.base != nullptr;
  const dim3 tb(SP_THREADS);
  if (A.ent_tiles) hipLaunchKernelGGL(k_sp_ent_count, dim3(A.ent_tiles), tb, 0, s, A, 0u);
  mark();
  hipLaunchKernelGGL(k_sp_front_scan, dim3(1), tb, 0, s, A, 0u);
  mark();
  if (A.ent_tiles) hipLaunchKernelGGL(k_sp_ent_count, dim3(A.ent_tiles), tb, 0, s, A, 1u);
  mark();
  if (A.tok_tiles) {
    if (inv) hipLaunchKernelGGL(k_sp_tok_runes<true>, dim3(A.tok_tiles), tb, 0, s, A);
    else hipLaunchKernelGGL(k_sp_tok_runes<false>, dim3(A.tok_tiles), tb, 0, s, A);
  }
  mark();
  hipLaunchKernelGGL(k_sp_front_scan, dim3(1), tb, 0, s, A, 1u);
  mark();
}
inline void sp_launch_front(const Args &A, hipStream_t s) { sp_launch_front(A, s, [] {}); }

}  // namespace
