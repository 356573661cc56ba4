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
// tiles of 256 list entries, tiles of 256 tokens, or one scanning block (four stages: k_sp_front_scan 0 and 1,
// k_sp_scan 2 and 3).  The first five launches are the front that dtk_streamoffs.hip shares (dtk_streampos_front.h):
//   k_sp_ent_count, scan 0, k_sp_ent_count   SentenceEnd calls and TextEnd entries in front of every entry; te_idx
//   k_sp_tok_runes, scan 1                   v, the text a token belongs to, its SentenceEnd calls; posC in front of a tile
//   k_sp_tok_weights, scan 2                 rstart / rend; the bytes of a token's surface, position and sentence integers
//   k_sp_ent_weights, scan 3                 the bytes of an entry (a TextEnd: its lines); lengths, carry_out, the trailer
//   k_sp_ent_offsets                         where every entry and every text's lines begin
//   k_sp_write                               surfaces and integers
// All kernels return at once when the list is longer than its arrays (the host packs it again and renders again; the
// carry slot is not written then), and none writes at or behind `cap`.
#include "dtk_streampos_front.h"

namespace {

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

// ---------------------------------------------------------------- tokens: rstart / rend and the weights
template <bool INV>
__global__ __launch_bounds__(256) void k_sp_tok_weights(Args A) {
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  uint32_t meta;
  const int64_t re = sp_tok_positions(A, k, wave_s, wave_f, meta);
  uint64_t w[3] = {0, 0, 0};
  if (k < N) {
    const int64_t rs = re - (int64_t)A.tok_len[k];
    if (A.bits & W_TOKENS) {
      const uint32_t be = sp_bend(A, k), bs = std::min(A.tok_bstart[k], be);
      w[0] = (uint64_t)(be - bs) + 1u;
      if (INV)
        for (uint32_t q = bs; q < be; q++) w[0] += sym_invalid_byte(A.sym, q) ? 2u : 0u;
    }
    const uint32_t ds = 1u + dec_len64(rs), de = 1u + dec_len64(re);
    if (A.bits & W_TOKEN_POS) w[1] = ds + de;
    if (A.bits & W_SENTENCE_POS) w[2] = ((meta >> 31) ? ds : 0u) + (uint64_t)(meta & 0x3FFFFFFFu) * de;
  }
#pragma unroll
  for (uint32_t r = 0; r < 3u; r++) {
    uint64_t tot;
    const uint64_t e = block_excl_scan64(w[r], wave_tot, tot);
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
  const uint32_t E = evl_entries(A);
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
      const uint32_t tl = lower_bound32(A.tok_bend, N, A.evl_pos[j]);  // (the token on this cursor begins the next text)
      const uint32_t tf = g ? lower_bound32(A.tok_bend, N, A.evl_pos[A.te_idx[g - 1u]]) : 0u;
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
  (void)block_excl_scan64(w, wave_tot, total);
  if (threadIdx.x == 0u) A.ent_base[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_sp_ent_offsets(Args A) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = evl_entries(A);
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
  const uint64_t x = block_excl_scan64(w, wave_tot, total);
  if (j >= E) return;
  const uint64_t at = A.ent_base[blockIdx.x] + x;
  A.ew[j] = at;
  if (kd & DTK_EVL_K_TEOT) {
    const DtkPosCarry c = *A.carry_in;
    const uint32_t g = (uint32_t)(A.cnt[j] >> 32);
    const uint32_t tl = lower_bound32(A.tok_bend, N, A.evl_pos[j]);
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
__global__ __launch_bounds__(256) void k_sp_scan(Args A, uint32_t stage) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) {
    if (stage == 2u && threadIdx.x == 0u) A.trailer->out_len = SP_NONE;
    return;
  }
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t s = (A.bits & W_SENTENCES) ? 1u : 0u;
  if (stage == 2u) {  // ---- the tokens' weights
    uint64_t tot[3];
    for (uint32_t r = 0; r < 3u; r++) tot[r] = scan_row64(A.w_base + (uint64_t)r * A.tok_tiles, A.tok_tiles, wave_tot);
    if (threadIdx.x == 0u)
      for (uint32_t r = 0; r < 3u; r++) A.hdr->tot[r] = tot[r];
    return;
  }
  // ---- stage 3: the entries' bytes, the lengths, the last text, the carry
  const uint64_t ent_tot = scan_row64(A.ent_base, A.ent_tiles, wave_tot);
  if (threadIdx.x != 0u) return;
  const DtkPosCarry c = *A.carry_in;
  const uint32_t tail = A.with_tail ? (A.doc_tail[0] & 3u) : 0u;
  const uint32_t n_te = A.hdr->n_te;
  A.ew[E] = ent_tot;
  A.hdr->ent_tot = ent_tot;
  const uint32_t g = n_te;
  const uint32_t tf = g ? lower_bound32(A.tok_bend, N, A.evl_pos[A.te_idx[g - 1u]]) : 0u;
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
  const DtkPosCarry o = sp_carry_out(A, c, E, tail, n_te, tf, L.stot != 0u);
  T.carry_in = c;
  T.carry_out = o;
  T.flags = A.hdr->flags;
  *A.trailer = T;
  *A.carry_out = o;
}

// ---------------------------------------------------------------- surfaces and integers
template <bool INV>
__global__ __launch_bounds__(256) void k_sp_write(Args A) {
  const uint32_t E = evl_entries(A);
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
    const uint32_t lbk = lower_bound32(A.evl_pos, E, be);
    uint64_t o = sp_w(A, 0u, k) + A.ew[lbk];
    if (lbk < E && A.evl_pos[lbk] == be) o += A.ent_pre[lbk];
    const uint8_t *__restrict__ text = A.text;
    for (uint32_t q = bs; q < be; q++) {
      if (INV && sym_invalid_byte(A.sym, q)) {
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
  sp_launch_front(A, s);
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