// dtk_streamoffs.hip -- the writer's rune offsets and sentence list of one slice of a stream as arrays
// (dtk_stream_set_offsets): what a NewTokenWriter with TOKEN_POS | SENTENCE_POS collects in pos[] and sent[]
// (token_writer.go:38-42) during the slice's calls, from the state its predecessor left in a carry slot (DtkPosCarry).
// The calls, the texts and the rules are dtk_streampos.hip's, and so is the front of the chain
// (dtk_streampos_front.h): the list's prefix counts and te_idx, k_sp_tok_runes, posC in front of every token tile.
// Behind it, where position rendering sizes and writes digits, this unit lays the integers out:
//   k_so_tok_place    rstart / rend; a token's sentence ints (rstart behind a SentenceEnd or TextEnd call, rend for every
//                     SentenceEnd call behind it) counted and scanned inside its tile of 256 tokens
//   k_so_scan         one block: the tiles' scan; the counts, the tail's text row, carry_out, the trailer
//   k_so_sent         sent[]: the head's ints (SentenceEnd calls in front of the first token push the carried posC), then
//                     every token's at head + tile + place
//   k_so_text         a row per TextEnd entry: tokens and sent ints of the slice in front of it
//   k_so_pack64       the blocked form (dtk_off_block64), one wave per block of 64 tokens
// Plain launches on the download stream behind k_evl_*, no block waits for another.  All kernels return at once when
// the list is longer than its arrays (the trailer says so, the carry slot is not written; the host packs the list again
// and launches again), and none writes at or behind a capacity.
#include "dtk_streampos_front.h"

namespace {

typedef DtkStreamOffsArgs OArgs;

// sentence ints of the slice in front of token k's (n_tok: all of them), behind k_so_scan
__device__ __forceinline__ uint64_t so_sent_at(const OArgs &O, uint32_t k) {
  const Args &A = O.front;
  const uint64_t head = A.hdr->head_n;
  return k < (uint32_t)A.n_tok ? head + O.sent_base[k >> 8] + O.sent_in[k] : head + A.hdr->tot[2];
}

__device__ __forceinline__ int64_t wave_min64(int64_t v) {
#pragma unroll
  for (uint32_t o = 1; o < WAVE; o <<= 1) v = std::min(v, (int64_t)__shfl_xor((long long)v, (int)o));
  return v;
}
__device__ __forceinline__ int64_t wave_max64(int64_t v) {
#pragma unroll
  for (uint32_t o = 1; o < WAVE; o <<= 1) v = std::max(v, (int64_t)__shfl_xor((long long)v, (int)o));
  return v;
}

// ---------------------------------------------------------------- tokens: rstart / rend, the place of the sentence ints
__global__ __launch_bounds__(256) void k_so_tok_place(OArgs O) {
  __shared__ int64_t wave_s[SP_WAVES];
  __shared__ uint32_t wave_f[SP_WAVES];
  __shared__ uint64_t wave_tot[SP_WAVES];
  const Args &A = O.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  uint32_t meta;
  (void)sp_tok_positions(A, k, wave_s, wave_f, meta);
  const uint64_t n = k < N ? (uint64_t)(meta >> 31) + (meta & 0x3FFFFFFFu) : 0u;
  uint64_t tot;
  const uint64_t e = block_excl_scan64(n, wave_tot, tot);
  if (k < N) O.sent_in[k] = (uint32_t)e;
  if (threadIdx.x == 0u) O.sent_base[blockIdx.x] = tot;
}

// ---------------------------------------------------------------- the scanning block
__global__ __launch_bounds__(256) void k_so_scan(OArgs O) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const Args &A = O.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) {
    if (threadIdx.x == 0u) O.trailer->n_tok = SP_NONE;
    return;
  }
  const uint32_t N = (uint32_t)A.n_tok;
  const uint64_t tok_ints = scan_row64(O.sent_base, A.tok_tiles, wave_tot);
  __syncthreads();  // (thread 0 reads the scan of another thread's tile)
  if (threadIdx.x != 0u) return;
  const DtkPosCarry c = *A.carry_in;
  const uint32_t tail = A.with_tail ? (A.doc_tail[0] & 3u) : 0u;
  const uint32_t n_te = A.hdr->n_te;
  A.hdr->tot[2] = tok_ints;
  const uint64_t n_sent = (uint64_t)A.hdr->head_n + tok_ints;
  // the text that is open behind the last TextEnd entry: its first token, its ints
  const uint32_t tf = n_te ? lower_bound32(A.tok_bend, N, A.evl_pos[A.te_idx[n_te - 1u]]) : 0u;
  const uint64_t open_ints = n_sent - (n_te ? so_sent_at(O, tf) : 0u);
  DtkOffsTrailer T{};
  T.n_tok = N;
  T.n_sent = n_sent;
  T.n_text = n_te;
  if (tail & DTK_TAIL_E) {  // the tail's TextEnd closes it
    if (n_te < O.text_cap) { O.text_tok_end[n_te] = N; O.text_sent_end[n_te] = (uint32_t)n_sent; }
    T.n_text++;
  }
  const DtkPosCarry o = sp_carry_out(A, c, E, tail, n_te, tf, open_ints != 0u);
  T.carry_in = c;
  T.carry_out = o;
  T.flags = A.hdr->flags;
  *O.trailer = T;
  *A.carry_out = o;
}

// ---------------------------------------------------------------- sent[]
__global__ __launch_bounds__(256) void k_so_sent(OArgs O) {
  const Args &A = O.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  int64_t *__restrict__ sent = O.sent;
  if (k == 0u) {
    const int64_t posC = A.carry_in->posC;
    const uint64_t n = std::min<uint64_t>(A.hdr->head_n, O.sent_cap);
    for (uint64_t i = 0; i < n; i++) sent[i] = posC;
  }
  if (k >= N) return;
  const uint32_t meta = A.tok_meta[k];
  uint64_t at = so_sent_at(O, k);
  if (meta >> 31) {
    if (at < O.sent_cap) sent[at] = A.rstart[k];
    at++;
  }
  const uint32_t n = meta & 0x3FFFFFFFu;
  const int64_t re = A.rend[k];
  for (uint32_t i = 0; i < n; i++, at++)
    if (at < O.sent_cap) sent[at] = re;
}

// ---------------------------------------------------------------- the text rows
__global__ __launch_bounds__(256) void k_so_text(OArgs O) {
  const Args &A = O.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t g = blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= A.hdr->n_te || g >= O.text_cap) return;
  const uint32_t tl = lower_bound32(A.tok_bend, N, A.evl_pos[A.te_idx[g]]);  // (the token on this cursor begins the next text)
  O.text_tok_end[g] = tl;
  O.text_sent_end[g] = (uint32_t)so_sent_at(O, tl);
}

// ---------------------------------------------------------------- the blocked form
// dtk_off_block64 (include/datok_gpu.h): k_pack_blk's rules on 64-bit offsets.  One wave per block of 64 tokens, one
// token per lane; lanes behind the last token take part in nothing.
__global__ __launch_bounds__(256) void k_so_pack64(OArgs O) {
  const Args &A = O.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint64_t N = A.n_tok;
  const uint32_t lane = lane_id();
  const uint64_t blk = (uint64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (blk * WAVE >= N) return;  // (wave-uniform)
  const uint64_t i = blk * WAVE + lane;
  const bool live = i < N;
  int64_t s = 0, e = 0;
  if (live) { s = A.rstart[i]; e = A.rend[i]; }
  // the first token of a new text starts before its predecessor's end: the block's one break
  const int64_t prev_e = (int64_t)__shfl_up((long long)e, 1);
  const unsigned long long dec = __ballot(live && lane != 0u && s < prev_e);
  const uint32_t brk = dec ? (uint32_t)__ffsll((long long)dec) - 1u : (uint32_t)WAVE;
  const bool seg1 = lane >= brk;
  const int64_t lo = live ? std::min(s, e) : INT64_MAX, hi = live ? std::max(s, e) : INT64_MIN;
  const int64_t lo0 = wave_min64(seg1 ? INT64_MAX : lo), hi0 = wave_max64(seg1 ? INT64_MIN : hi);  // (lane 0 is live)
  int64_t lo1 = 0, hi1 = 0;
  if (brk < WAVE) { lo1 = wave_min64(seg1 ? lo : INT64_MAX); hi1 = wave_max64(seg1 ? hi : INT64_MIN); }  // (lane brk is live)
  const int64_t base = seg1 ? lo1 : lo0;
  if (live) O.words[i] = ((uint32_t)(s - base) & 0xFFFFu) | ((uint32_t)(e - base) << 16);
  if (lane == 0u) {
    O.heads[blk] = DtkOffBlock64{lo0, lo1, brk, 0u};
    if (hi0 - lo0 > (int64_t)O.span || hi1 - lo1 > (int64_t)O.span) O.trailer->blk_fail = 1u;  // (behind k_so_scan's store of the block)
  }
}

}  // namespace

// Lays the workspace out in `ws` (64-bit words; null: only the size is wanted) and returns its words.
extern "C" uint64_t dtk_streamoffs_ws(struct DtkStreamOffsArgs *o, uint64_t *ws) {
  DtkStreamPosArgs *a = &o->front;
  const uint64_t N = a->n_tok, R = a->evl_cap, tt = a->tok_tiles, et = a->ent_tiles;
  uint64_t at = 0;
  auto take = [&](uint64_t words) { uint64_t *p = ws ? ws + at : nullptr; at += words; return p; };
  a->hdr = reinterpret_cast<DtkPosHdr *>(take((sizeof(DtkPosHdr) + 7u) / 8u));
  a->ent_base = take(et);
  a->cnt = take(R + 1u);
  a->tile_sum = reinterpret_cast<int64_t *>(take(tt));
  a->tile_in = reinterpret_cast<int64_t *>(take(tt));
  o->sent_base = take(tt);
  a->te_idx = reinterpret_cast<uint32_t *>(take(words32(R)));
  a->tile_flag = reinterpret_cast<uint32_t *>(take(words32(tt)));
  a->tok_v = reinterpret_cast<int32_t *>(take(words32(N)));
  a->tok_len = reinterpret_cast<uint32_t *>(take(words32(N)));
  a->tok_meta = reinterpret_cast<uint32_t *>(take(words32(N)));
  a->tok_seg = reinterpret_cast<uint32_t *>(take(words32(N)));
  o->sent_in = reinterpret_cast<uint32_t *>(take(words32(N)));
  return at;
}

// events: null, or DTK_STREAMOFFS_EVENTS events that are recorded in front of the first launch and behind each of the
// ten (a launch that is left out records too): the per-launch times of scripts/stream_offsets.py.
extern "C" int dtk_launch_streamoffs(const DtkStreamOffsArgs *args, void *stream, void **events) {
  OArgs O = *args;
  const Args &A = O.front;
  hipStream_t s = (hipStream_t)stream;
  if (A.n_tok >= 0x80000000ull || A.tok_tiles != dtk_streamrender_tiles(A.n_tok) ||
      A.ent_tiles != dtk_streamrender_tiles(A.evl_cap) || (A.bits & ~W_NEWLINE) != (W_TOKEN_POS | W_SENTENCE_POS) ||
      !A.hdr || !A.carry_in || !A.carry_out || A.carry_in == A.carry_out || !O.trailer || !O.sent_base ||
      (A.n_tok && (!A.rstart || !A.rend || !O.sent_in)) || !O.sent || !O.text_tok_end || !O.text_sent_end ||
      (O.blocked && A.n_tok && (!O.words || !O.heads)))
    return 1;
  const dim3 tb(SP_THREADS);
  uint32_t n_marks = 0;
  auto mark = [&] {
    if (events && n_marks < DTK_STREAMOFFS_EVENTS) (void)hipEventRecord((hipEvent_t)events[n_marks], s);
    n_marks++;
  };
  mark();
  sp_launch_front(A, s, mark);
  if (A.tok_tiles) hipLaunchKernelGGL(k_so_tok_place, dim3(A.tok_tiles), tb, 0, s, O);
  mark();
  hipLaunchKernelGGL(k_so_scan, dim3(1), tb, 0, s, O);
  mark();
  hipLaunchKernelGGL(k_so_sent, dim3(A.tok_tiles ? A.tok_tiles : 1u), tb, 0, s, O);
  mark();
  if (A.ent_tiles) hipLaunchKernelGGL(k_so_text, dim3(A.ent_tiles), tb, 0, s, O);
  mark();
  if (O.blocked && A.n_tok)
    hipLaunchKernelGGL(k_so_pack64, dim3((unsigned)((A.n_tok + SP_THREADS - 1u) / SP_THREADS)), tb, 0, s, O);
  mark();
  return (int)hipGetLastError();
}
