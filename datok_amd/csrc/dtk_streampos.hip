// dtk_streampos.hip -- the bytes of NewTokenWriter(w, bits) for one slice of a stream in a mode with TOKEN_POS or
// SENTENCE_POS (dtk_stream_set_position_render).  The writer's state runs across cuts (token_writer.go:38-42): a slice
// reads it from its predecessor's carry slot and leaves its own in another (DtkPosCarry), so the slices chain on the
// device, in the order they are enqueued on the download stream.
//
// The calls are those of dtk_streamrender.hip: the slice's tokens merged with its event list by cursor (SEOT, TEOT, the
// token that ends there, SEPS), the tail word's on the stream's last slice.  The TextEnd calls cut the slice's tokens
// into texts ("segments"); text g is closed by the g-th TEOT entry, the last one by the tail's TextEnd or not at all.
//   Token k:  B is the end of token k - 1 (the slice's `first` for token 0), for a matrix model the cursor of the last
//             TextEnd in front of it if that lies behind.  It adds v = runes[B, bend) to posC, one less where the
//             newline rule fires: rend is a sum of v over the text's tokens -- a scan segmented at the tokens that begin
//             a text, seeded with the carried posC -- and rstart = rend - runes[bstart, bend).
//             It pushes rstart and rend to pos, rstart to sent if a SentenceEnd or TextEnd call lies between it and its
//             predecessor (or the carry says so), and every SentenceEnd call behind it, up to the next Token or
//             TextEnd, pushes its rend to sent: all integers of a text belong to one of its tokens, except those of
//             SentenceEnd calls at the head of the slice, which push the carried posC ("head").
//   Lines:    an integer is written as a blank and its digits; the first of a line that holds no integer of an earlier
//             slice drops the blank.  A closed line ends in '\n', which like every other byte that is neither a surface
//             byte nor part of an integer comes from the host's fill.  The integers of the text still open at the cut
//             are written behind the output: the open fragments.
//
// Plain launches on the download stream behind k_evl_*, no block waits for another; every kernel is one of three kinds,
// tiles of 256 list entries, tiles of 256 tokens, or one scanning block (k_sp_scan, four stages):
//   k_sp_ent_count, scan 0, k_sp_ent_index   SentenceEnd calls and TextEnd entries in front of every entry; te_idx
//   k_sp_tok_runes, scan 1                   v, the text a token belongs to, its SentenceEnd calls; posC in front of a tile
//   k_sp_tok_weights, scan 2                 rstart / rend; the bytes of a token's surface, position and sentence integers
//   k_sp_ent_weights, scan 3                 the bytes of an entry (a TextEnd: its lines); lengths, carry_out, the trailer
//   k_sp_ent_offsets                         where every entry and every text's lines begin
//   k_sp_write                               surfaces and integers
// All kernels return at once when the list is longer than its arrays (the host packs it again and renders again; the
// carry slot is not written then), and none writes at or behind `cap`.
#include <algorithm>

#include "dtk_device.h"

namespace {

constexpr uint32_t SP_THREADS = 256;
constexpr uint32_t SP_WAVES = SP_THREADS / WAVE;
constexpr uint32_t W_TOKENS = 1u, W_SENTENCES = 2u, W_TOKEN_POS = 4u, W_SENTENCE_POS = 8u, W_NEWLINE = 16u;
constexpr uint64_t SP_NONE = ~0ull;

typedef DtkStreamPosArgs Args;

__device__ __forceinline__ uint32_t sp_entries(const Args &A) {
  const uint32_t n = *A.evl_count;
  return n > A.evl_cap ? 0xFFFFFFFFu : n;
}

// first i in [0, n) with a[i] >= x, else n
__device__ __forceinline__ uint32_t sp_lower(const uint32_t *__restrict__ a, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t sp_bend(const Args &A, uint32_t k) { return std::min(A.tok_bend[k], A.text_len); }

// exclusive prefix sum of a 64-bit value over the block's 256 threads (as sr_block_excl of dtk_streamrender.hip)
__device__ __forceinline__ uint64_t sp_block_excl(uint64_t v, uint64_t *wave_tot, uint64_t &total) {
  const uint64_t inc = wave_incl_scan64(v);
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane_id() == WAVE - 1u) wave_tot[wave] = inc;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < SP_WAVES; k++) {
    const uint64_t t = wave_tot[k];
    before += k < wave ? t : 0u;
    total += t;
  }
  return before + inc - v;
}

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

__device__ __forceinline__ bool sp_invalid(const DtkSym &S, uint64_t i) {  // as sr_invalid
  const uint32_t e = dtk_sym_entry(S, i);
  return DTK_SYM_WIDTH(e) == 1u && ((e >> DTK_SYM_CLS_SHIFT) & 3u) >= 2u;
}

// SentenceEnd calls from entry `ap` on (and `seps` in front of it) up to the next TextEnd or the token `next` (n_tok:
// none), whichever comes first; the tail's SentenceEnd if neither does
__device__ __forceinline__ uint32_t sp_sent_calls(const Args &A, uint32_t E, uint32_t ap, uint32_t seps, uint32_t next) {
  const uint32_t N = (uint32_t)A.n_tok;
  uint32_t b = E;
  bool atb = false;
  if (next < N) {
    const uint32_t bn = sp_bend(A, next);
    b = sp_lower(A.evl_pos, E, bn);
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

// a weight's exclusive scan over the tokens (r: 0 surfaces, 1 position integers, 2 sentence integers), behind scan 2
__device__ __forceinline__ uint64_t sp_w(const Args &A, uint32_t r, uint32_t k) {
  const uint32_t N = (uint32_t)A.n_tok;
  return k < N ? A.w_base[(uint64_t)r * A.tok_tiles + (k >> 8)] + A.w_in[(uint64_t)r * N + k] : A.hdr->tot[r];
}

// The lines of the TextEnd that closes text g = tokens [tf, tl): their bytes in the output, and the bytes of their
// integers written as blank + digits
struct SpLines { uint64_t pbytes, sbytes, ptot, stot; };
__device__ __forceinline__ SpLines sp_lines(const Args &A, const DtkPosCarry &c, uint32_t g, uint32_t tf, uint32_t tl) {
  SpLines L{0, 0, 0, 0};
  if (A.bits & W_TOKEN_POS) {
    const bool cont = g == 0u && c.pos_nonempty;
    L.ptot = sp_w(A, 1u, tl) - sp_w(A, 1u, tf);
    if (tl > tf || cont) L.pbytes = L.ptot + (cont ? 1u : 0u);  // (a line of its own: no blank in front, '\n' behind)
  }
  if (A.bits & W_SENTENCE_POS) {
    const bool cont = g == 0u && c.sent_nonempty;
    L.stot = sp_w(A, 2u, tl) - sp_w(A, 2u, tf) + (g == 0u ? A.hdr->head_w : 0u);
    if (L.stot || cont) L.sbytes = L.stot + (cont ? 1u : 0u);
  }
  return L;
}

// the integer at byte `rel` of a line's blank + digits form; fresh: the line's first integer drops its blank
__device__ __forceinline__ void sp_put(const Args &A, uint64_t line, uint64_t rel, bool fresh, int64_t v) {
  uint64_t o = line + rel;
  if (fresh) {
    if (rel) { o--; if (o < A.cap) A.out[o] = ' '; o++; }
  } else {
    if (o < A.cap) A.out[o] = ' ';
    o++;
  }
  dec_put64(A.out, o, A.cap, v, dec_len64(v));
}

// ---------------------------------------------------------------- the list's prefix counts
__global__ __launch_bounds__(256) void k_sp_ent_count(Args A) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t j = blockIdx.x * SP_THREADS + threadIdx.x;
  uint64_t v = 0;
  if (j < E) {
    const uint32_t kd = A.evl_kind[j];
    v = (uint64_t)(((kd & DTK_EVL_K_SEOT) ? 1u : 0u) + ((kd & DTK_EVL_K_SEPS) ? 1u : 0u)) | ((kd & DTK_EVL_K_TEOT) ? 1ull << 32 : 0ull);
  }
  uint64_t total;
  const uint64_t x = sp_block_excl(v, wave_tot, total);
  if (A.ew && j < E) A.cnt[j] = A.ent_base[blockIdx.x] + x;  // (second launch: k_sp_ent_index)
  if (A.ew && j < E && (v >> 32)) A.te_idx[(uint32_t)((A.ent_base[blockIdx.x] + x) >> 32)] = j;
  if (!A.ew && threadIdx.x == 0u) A.ent_base[blockIdx.x] = total;
}

// ---------------------------------------------------------------- tokens: runes and calls
template <bool INV>
__global__ __launch_bounds__(256) void k_sp_tok_runes(Args A) {
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  Seg x{0, 0u};
  if (k < N) {
    const DtkPosCarry c = *A.carry_in;
    const uint32_t be = sp_bend(A, k), bs = std::min(A.tok_bstart[k], be);
    const uint32_t lbk = sp_lower(A.evl_pos, E, be);
    const uint32_t kd = (lbk < E && A.evl_pos[lbk] == be) ? A.evl_kind[lbk] : 0u;  // the entry on the token's cursor
    const uint32_t te_k = (uint32_t)(A.cnt[lbk] >> 32) + ((kd & DTK_EVL_K_TEOT) ? 1u : 0u);
    uint32_t te_p = 0, between, bp = A.first;
    if (k) {
      bp = sp_bend(A, k - 1u);
      const uint32_t lbp = sp_lower(A.evl_pos, E, bp);
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

// ---------------------------------------------------------------- tokens: rstart / rend and the weights
template <bool INV>
__global__ __launch_bounds__(256) void k_sp_tok_weights(Args A) {
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  Seg x{0, 0u};
  uint32_t meta = 0;
  if (k < N) {
    meta = A.tok_meta[k];
    x.s = A.tok_v[k];
    x.f = (meta >> 30) & 1u;
  }
  Seg total;
  const int64_t re = seg_block_incl(x, Seg{A.tile_in[blockIdx.x], 0u}, wave_s, wave_f, total).s;
  uint64_t w[3] = {0, 0, 0};
  if (k < N) {
    const int64_t rs = re - (int64_t)A.tok_len[k];
    A.rstart[k] = rs;
    A.rend[k] = re;
    if ((A.bits & W_NEWLINE) && re == 0) atomicOr(&A.hdr->flags, 1u);
    if (A.bits & W_TOKENS) {
      const uint32_t be = sp_bend(A, k), bs = std::min(A.tok_bstart[k], be);
      w[0] = (uint64_t)(be - bs) + 1u;
      if (INV)
        for (uint32_t q = bs; q < be; q++) w[0] += sp_invalid(A.sym, q) ? 2u : 0u;
    }
    const uint32_t ds = 1u + dec_len64(rs), de = 1u + dec_len64(re);
    if (A.bits & W_TOKEN_POS) w[1] = ds + de;
    if (A.bits & W_SENTENCE_POS) w[2] = ((meta >> 31) ? ds : 0u) + (uint64_t)(meta & 0x3FFFFFFFu) * de;
  }
#pragma unroll
  for (uint32_t r = 0; r < 3u; r++) {
    uint64_t tot;
    const uint64_t e = sp_block_excl(w[r], wave_tot, tot);
    if (k < N) A.w_in[(uint64_t)r * N + k] = (uint32_t)e;
    if (threadIdx.x == 0u) {
      A.w_base[(uint64_t)r * A.tok_tiles + blockIdx.x] = tot;
      if (tot >> 32) atomicOr(&A.hdr->flags, 2u);  // (w_in holds 32 bits: the host ends the run)
    }
  }
}

// ---------------------------------------------------------------- entries: bytes
__global__ __launch_bounds__(256) void k_sp_ent_weights(Args A) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t j = blockIdx.x * SP_THREADS + threadIdx.x;
  const uint32_t s = (A.bits & W_SENTENCES) ? 1u : 0u;
  uint64_t w = 0;
  if (j < E) {
    const uint32_t kd = A.evl_kind[j];
    uint64_t pre = (kd & DTK_EVL_K_SEOT) ? s : 0u;
    if (kd & DTK_EVL_K_TEOT) {
      const DtkPosCarry c = *A.carry_in;
      const uint32_t g = (uint32_t)(A.cnt[j] >> 32);
      const uint32_t tl = sp_lower(A.tok_bend, N, A.evl_pos[j]);  // (the token on this cursor begins the next text)
      const uint32_t tf = g ? sp_lower(A.tok_bend, N, A.evl_pos[A.te_idx[g - 1u]]) : 0u;
      const SpLines L = sp_lines(A, c, g, tf, tl);
      A.seg_pw0[g] = sp_w(A, 1u, tf);
      A.seg_sw0[g] = (int64_t)sp_w(A, 2u, tf) - (g == 0u ? (int64_t)A.hdr->head_w : 0);
      A.seg_sent[g] = L.pbytes;  // (k_sp_ent_offsets adds where the lines begin)
      pre += L.pbytes + L.sbytes;
    }
    A.ent_pre[j] = pre;
    w = pre + ((kd & DTK_EVL_K_SEPS) ? s : 0u);
  }
  uint64_t total;
  (void)sp_block_excl(w, wave_tot, total);
  if (threadIdx.x == 0u) A.ent_base[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_sp_ent_offsets(Args A) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t j = blockIdx.x * SP_THREADS + threadIdx.x;
  const uint32_t s = (A.bits & W_SENTENCES) ? 1u : 0u;
  uint32_t kd = 0;
  uint64_t w = 0;
  if (j < E) {
    kd = A.evl_kind[j];
    w = A.ent_pre[j] + ((kd & DTK_EVL_K_SEPS) ? s : 0u);
  }
  uint64_t total;
  const uint64_t x = sp_block_excl(w, wave_tot, total);
  if (j >= E) return;
  const uint64_t at = A.ent_base[blockIdx.x] + x;
  A.ew[j] = at;
  if (kd & DTK_EVL_K_TEOT) {
    const DtkPosCarry c = *A.carry_in;
    const uint32_t g = (uint32_t)(A.cnt[j] >> 32);
    const uint32_t tl = sp_lower(A.tok_bend, N, A.evl_pos[j]);
    const uint64_t line = sp_w(A, 0u, tl) + at + ((kd & DTK_EVL_K_SEOT) ? s : 0u);
    const uint64_t pb = A.seg_sent[g];
    A.seg_pos[g] = line;
    A.seg_sent[g] = line + pb;
    if (g == 0u) {  // the text that began in an earlier slice: its held integers belong in front of these lines
      if ((A.bits & W_TOKEN_POS) && c.pos_nonempty) A.trailer->splice_pos = line;
      if ((A.bits & W_SENTENCE_POS) && c.sent_nonempty) A.trailer->splice_sent = line + pb;
    }
  }
}

// ---------------------------------------------------------------- the scanning block
// exclusive scan of base[0 .. n) in place; returns the sum
__device__ __forceinline__ uint64_t sp_scan_row(uint64_t *base, uint32_t n, uint64_t *wave_tot) {
  uint64_t carry = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += SP_THREADS) {  // (block-uniform trip count)
    const uint32_t i = i0 + threadIdx.x;
    const uint64_t v = i < n ? base[i] : 0u;
    uint64_t total;
    const uint64_t x = sp_block_excl(v, wave_tot, total);
    if (i < n) base[i] = carry + x;
    carry += total;
  }
  return carry;
}

__global__ __launch_bounds__(256) void k_sp_scan(Args A, uint32_t stage) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) {
    if (stage == 0u && threadIdx.x == 0u) A.trailer->out_len = SP_NONE;
    return;
  }
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t s = (A.bits & W_SENTENCES) ? 1u : 0u;
  if (stage == 0u) {  // ---- the entries' counts
    const uint64_t sum = sp_scan_row(A.ent_base, A.ent_tiles, wave_tot);
    if (threadIdx.x != 0u) return;
    A.cnt[E] = sum;
    DtkPosHdr h{};
    h.n_te = (uint32_t)(sum >> 32);
    *A.hdr = h;
    return;
  }
  if (stage == 1u) {  // ---- posC in front of every token tile; the head's SentenceEnd calls
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
    return;
  }
  if (stage == 2u) {  // ---- the tokens' weights
    uint64_t tot[3];
    for (uint32_t r = 0; r < 3u; r++) tot[r] = sp_scan_row(A.w_base + (uint64_t)r * A.tok_tiles, A.tok_tiles, wave_tot);
    if (threadIdx.x == 0u)
      for (uint32_t r = 0; r < 3u; r++) A.hdr->tot[r] = tot[r];
    return;
  }
  // ---- stage 3: the entries' bytes, the lengths, the last text, the carry
  const uint64_t ent_tot = sp_scan_row(A.ent_base, A.ent_tiles, wave_tot);
  if (threadIdx.x != 0u) return;
  const DtkPosCarry c = *A.carry_in;
  const uint32_t tail = A.with_tail ? (A.doc_tail[0] & 3u) : 0u;
  const uint32_t n_te = A.hdr->n_te;
  A.ew[E] = ent_tot;
  A.hdr->ent_tot = ent_tot;
  const uint32_t g = n_te;
  const uint32_t tf = g ? sp_lower(A.tok_bend, N, A.evl_pos[A.te_idx[g - 1u]]) : 0u;
  const SpLines L = sp_lines(A, c, g, tf, N);
  A.seg_pw0[g] = sp_w(A, 1u, tf);
  A.seg_sw0[g] = (int64_t)sp_w(A, 2u, tf) - (g == 0u ? (int64_t)A.hdr->head_w : 0);
  const uint64_t base = A.hdr->tot[0] + ent_tot + ((tail & DTK_TAIL_S) ? s : 0u);
  DtkPosTrailer T{};
  T.splice_pos = T.splice_sent = SP_NONE;
  const bool contp = g == 0u && c.pos_nonempty, conts = g == 0u && c.sent_nonempty;
  if (tail & DTK_TAIL_E) {
    T.out_len = base + L.pbytes + L.sbytes;
    A.seg_pos[g] = base;
    A.seg_sent[g] = base + L.pbytes;
    if ((A.bits & W_TOKEN_POS) && contp) T.splice_pos = base;
    if ((A.bits & W_SENTENCE_POS) && conts) T.splice_sent = base + L.pbytes;
  } else {
    T.out_len = base;
    T.open_pos_len = L.ptot - ((L.ptot && !contp) ? 1u : 0u);
    T.open_sent_len = L.stot - ((L.stot && !conts) ? 1u : 0u);
    A.seg_pos[g] = base;
    A.seg_sent[g] = base + T.open_pos_len;
  }
  // the writer behind the slice's last call
  DtkPosCarry o{};
  const bool closed = (tail & DTK_TAIL_E) != 0u;
  o.posC = closed ? 0 : (N > tf ? A.rend[N - 1u] : (n_te ? 0 : c.posC));
  o.pos_nonempty = (!closed && (N > tf || contp)) ? 1u : 0u;
  o.init = (c.init && N == 0u) ? 1u : 0u;
  if (A.bits & W_SENTENCE_POS) {
    uint32_t after = E + tail;  // calls behind the last token
    if (N) {
      const uint32_t be = sp_bend(A, N - 1u);
      const uint32_t lbk = sp_lower(A.evl_pos, E, be);
      const uint32_t kd = (lbk < E && A.evl_pos[lbk] == be) ? A.evl_kind[lbk] : 0u;
      after = (E - lbk - (kd ? 1u : 0u)) + ((kd & DTK_EVL_K_SEPS) ? 1u : 0u) + tail;
    }
    o.sentB = (N ? after != 0u : (c.sentB || after != 0u)) ? 1u : 0u;
    o.sent_nonempty = (!closed && (L.stot || conts)) ? 1u : 0u;
  } else {  // (token_writer.go:60-63 runs in every position mode; nothing sets sentB again or clears sent)
    o.sentB = (c.sentB && N == 0u) ? 1u : 0u;
    o.sent_nonempty = (c.sent_nonempty || (c.sentB && N)) ? 1u : 0u;
  }
  T.carry_in = c;
  T.carry_out = o;
  T.flags = A.hdr->flags;
  *A.trailer = T;
  *A.carry_out = o;
}

// ---------------------------------------------------------------- surfaces and integers
template <bool INV>
__global__ __launch_bounds__(256) void k_sp_write(Args A) {
  const uint32_t E = sp_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  const DtkPosCarry c = *A.carry_in;
  uint8_t *__restrict__ out = A.out;
  if (k == 0u && (A.bits & W_SENTENCE_POS)) {  // the head's integers open text 0's sentence line
    const uint32_t n = A.hdr->head_n;
    const uint64_t step = 1u + dec_len64(c.posC);
    for (uint32_t i = 0; i < n; i++) sp_put(A, A.seg_sent[0], (uint64_t)i * step, !c.sent_nonempty, c.posC);
  }
  if (k >= N) return;
  const uint32_t g = A.tok_seg[k];
  const int64_t rs = A.rstart[k], re = A.rend[k];
  const uint32_t ds = 1u + dec_len64(rs), de = 1u + dec_len64(re);
  if (A.bits & W_TOKENS) {
    const uint32_t be = sp_bend(A, k), bs = std::min(A.tok_bstart[k], be);
    const uint32_t lbk = sp_lower(A.evl_pos, E, be);
    uint64_t o = sp_w(A, 0u, k) + A.ew[lbk];
    if (lbk < E && A.evl_pos[lbk] == be) o += A.ent_pre[lbk];
    const uint8_t *__restrict__ text = A.text;
    for (uint32_t q = bs; q < be; q++) {
      if (INV && sp_invalid(A.sym, q)) {
        if (o + 3u <= A.cap) { out[o] = 0xEF; out[o + 1] = 0xBF; out[o + 2] = 0xBD; }
        o += 3u;
      } else {
        if (o < A.cap) out[o] = text[q];
        o += 1u;
      }
    }
  }
  if (A.bits & W_TOKEN_POS) {
    const bool fresh = !(g == 0u && c.pos_nonempty);
    const uint64_t rel = sp_w(A, 1u, k) - A.seg_pw0[g];
    sp_put(A, A.seg_pos[g], rel, fresh, rs);
    sp_put(A, A.seg_pos[g], rel + ds, fresh, re);
  }
  if (A.bits & W_SENTENCE_POS) {
    const uint32_t meta = A.tok_meta[k];
    const bool fresh = !(g == 0u && c.sent_nonempty);
    uint64_t rel = (uint64_t)((int64_t)sp_w(A, 2u, k) - A.seg_sw0[g]);
    if (meta >> 31) { sp_put(A, A.seg_sent[g], rel, fresh, rs); rel += ds; }
    const uint32_t n = meta & 0x3FFFFFFFu;
    for (uint32_t i = 0; i < n; i++) { sp_put(A, A.seg_sent[g], rel, fresh, re); rel += de; }
  }
}

inline uint64_t words32(uint64_t n) { return (n + 1u) / 2u; }

}  // namespace

// Lays the workspace out in `ws` (64-bit words; null: only the size is wanted) and returns its words.
extern "C" uint64_t dtk_streampos_ws(struct DtkStreamPosArgs *a, uint64_t *ws) {
  const uint64_t N = a->n_tok, R = a->evl_cap, tt = a->tok_tiles, et = a->ent_tiles;
  uint64_t at = 0;
  auto take = [&](uint64_t words) { uint64_t *p = ws ? ws + at : nullptr; at += words; return p; };
  a->hdr = reinterpret_cast<DtkPosHdr *>(take((sizeof(DtkPosHdr) + 7u) / 8u));
  a->ent_base = take(et);
  a->cnt = take(R + 1u);
  a->ew = take(R + 1u);
  a->ent_pre = take(R);
  a->seg_pos = take(R + 2u);
  a->seg_sent = take(R + 2u);
  a->seg_pw0 = take(R + 2u);
  a->seg_sw0 = reinterpret_cast<int64_t *>(take(R + 2u));
  a->tile_sum = reinterpret_cast<int64_t *>(take(tt));
  a->tile_in = reinterpret_cast<int64_t *>(take(tt));
  a->w_base = take(3u * tt);
  a->rstart = reinterpret_cast<int64_t *>(take(N));
  a->rend = reinterpret_cast<int64_t *>(take(N));
  a->te_idx = reinterpret_cast<uint32_t *>(take(words32(R)));
  a->tile_flag = reinterpret_cast<uint32_t *>(take(words32(tt)));
  a->tok_v = reinterpret_cast<int32_t *>(take(words32(N)));
  a->tok_len = reinterpret_cast<uint32_t *>(take(words32(N)));
  a->tok_meta = reinterpret_cast<uint32_t *>(take(words32(N)));
  a->tok_seg = reinterpret_cast<uint32_t *>(take(words32(N)));
  a->w_in = reinterpret_cast<uint32_t *>(take(words32(3u * N)));
  return at;
}

extern "C" int dtk_launch_streampos(const DtkStreamPosArgs *args, void *stream) {
  Args A = *args;
  hipStream_t s = (hipStream_t)stream;
  if (A.n_tok >= 0x80000000ull || A.tok_tiles != dtk_streamrender_tiles(A.n_tok) ||
      A.ent_tiles != dtk_streamrender_tiles(A.evl_cap) || (A.bits & ~31u) || !(A.bits & (W_TOKEN_POS | W_SENTENCE_POS)) ||
      !A.hdr || !A.carry_in || !A.carry_out || A.carry_in == A.carry_out || !A.trailer)
    return 1;
  const bool inv = A.sym.base != nullptr;
  const dim3 tb(SP_THREADS);
  if (A.ent_tiles) {
    Args C = A;
    C.ew = nullptr;  // (k_sp_ent_count's first launch: tile sums only)
    hipLaunchKernelGGL(k_sp_ent_count, dim3(A.ent_tiles), tb, 0, s, C);
  }
  hipLaunchKernelGGL(k_sp_scan, dim3(1), tb, 0, s, A, 0u);
  if (A.ent_tiles) hipLaunchKernelGGL(k_sp_ent_count, dim3(A.ent_tiles), tb, 0, s, A);
  if (A.tok_tiles) {
    if (inv) hipLaunchKernelGGL(k_sp_tok_runes<true>, dim3(A.tok_tiles), tb, 0, s, A);
    else hipLaunchKernelGGL(k_sp_tok_runes<false>, dim3(A.tok_tiles), tb, 0, s, A);
  }
  hipLaunchKernelGGL(k_sp_scan, dim3(1), tb, 0, s, A, 1u);
  if (A.tok_tiles) {
    if (inv) hipLaunchKernelGGL(k_sp_tok_weights<true>, dim3(A.tok_tiles), tb, 0, s, A);
    else hipLaunchKernelGGL(k_sp_tok_weights<false>, dim3(A.tok_tiles), tb, 0, s, A);
  }
  hipLaunchKernelGGL(k_sp_scan, dim3(1), tb, 0, s, A, 2u);
  if (A.ent_tiles) hipLaunchKernelGGL(k_sp_ent_weights, dim3(A.ent_tiles), tb, 0, s, A);
  hipLaunchKernelGGL(k_sp_scan, dim3(1), tb, 0, s, A, 3u);
  if (A.ent_tiles) hipLaunchKernelGGL(k_sp_ent_offsets, dim3(A.ent_tiles), tb, 0, s, A);
  const uint32_t wt = A.tok_tiles ? A.tok_tiles : 1u;
  if (inv) hipLaunchKernelGGL(k_sp_write<true>, dim3(wt), tb, 0, s, A);
  else hipLaunchKernelGGL(k_sp_write<false>, dim3(wt), tb, 0, s, A);
  return (int)hipGetLastError();
}
