// dtk_streamsens.hip -- the sentences of one slice of a stream as rows (dtk_stream_set_sentences): which tokens form a
// sentence, its byte span in the stream and its rune span in the writer's offsets.  A sentence is a maximal run of Token
// calls with no SentenceEnd or TextEnd between them, over the whole stream; a row is delivered by the slice whose calls
// close it, and the row that is open at a cut crosses it in a carry slot (DtkSenCarry) beside the writer's.
// The kernels run behind the offsets chain of the slice (dtk_streamoffs.hip) and read what it left on the device:
// tok_meta bit 31 marks a token that begins a sentence (sentB at the token), rstart / rend are the writer's offsets, the
// writer's carry_out says whether a sentence is open behind the slice's last call.
//   k_ss_count   the sentence-first tokens of a tile of 256 tokens: a ballot word per wave, the tile's sum
//   k_ss_scan    one block: the tiles' scan; the row count, the trailer, the tail's text row, the carry, the carried
//                row's start and the last row's end
//   k_ss_write   a sentence-first token opens its row and closes the row in front of it
//   k_ss_text    a row per TextEnd entry: rows of the slice closed in front of it
// Plain launches on the download stream, no block waits for another.  All kernels return at once when the list is longer
// than its arrays (the trailer says so, the carry slot is not written), and none writes at or behind a capacity.
#include "dtk_streampos_front.h"

namespace {

typedef DtkStreamSensArgs SArgs;

// sentence-first tokens of the slice in front of token k (n_tok: all of them), behind k_ss_scan
__device__ __forceinline__ uint64_t ss_firsts_before(const SArgs &S, uint32_t k) {
  if (k >= (uint32_t)S.front.n_tok) return S.trailer->firsts;
  uint64_t n = S.first_base[k >> 8];
  for (uint32_t w = (k >> 8) * SP_WAVES; w < (k >> 6); w++) n += popc(S.first_mask[w]);
  return n + popc(S.first_mask[k >> 6] & ((1ull << (k & 63u)) - 1ull));
}

// ---------------------------------------------------------------- tokens: who begins a sentence
__global__ __launch_bounds__(256) void k_ss_count(SArgs S) {
  __shared__ uint32_t wave_n[SP_WAVES];
  const Args &A = S.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  const unsigned long long m = __ballot(k < N && (A.tok_meta[k] >> 31));
  if (lane_id() == 0u) {
    if (k < N) S.first_mask[k >> 6] = m;
    wave_n[threadIdx.x >> 6] = popc(m);
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint64_t n = 0;
#pragma unroll
    for (uint32_t w = 0; w < SP_WAVES; w++) n += wave_n[w];
    S.first_base[blockIdx.x] = n;
  }
}

// ---------------------------------------------------------------- the scanning block
__global__ __launch_bounds__(256) void k_ss_scan(SArgs S) {
  __shared__ uint64_t wave_tot[SP_WAVES];
  const Args &A = S.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) {
    if (threadIdx.x == 0u) S.trailer->n_tok = SP_NONE;
    return;
  }
  const uint32_t N = (uint32_t)A.n_tok;
  const uint64_t firsts = scan_row64(S.first_base, A.tok_tiles, wave_tot);
  if (threadIdx.x != 0u) return;
  const DtkSenCarry ci = *S.carry_in;
  const uint64_t open_in = ci.open ? 1u : 0u;
  const uint32_t tail = A.with_tail ? (A.doc_tail[0] & 3u) : 0u;
  const uint32_t n_te = A.hdr->n_te;
  // (the writer behind the slice's last call, as k_so_scan left it: a token was the last call, or none came at all)
  const uint64_t rows = open_in + firsts;
  const bool still = !A.carry_out->sentB && !A.with_tail && rows != 0u;
  const uint64_t n_sen = rows - (still ? 1u : 0u);
  DtkSensTrailer T{};
  T.n_tok = N;
  T.n_sen = n_sen;
  T.n_text = n_te;
  T.firsts = firsts;
  T.flags = A.hdr->flags;
  if (tail & DTK_TAIL_E) {  // the tail's TextEnd: every row is closed in front of it
    if (n_te < S.text_cap) S.text_sen_end[n_te] = (uint32_t)n_sen;
    T.n_text++;
  }
  // where the slice's last token ends (none: where the carried row's last one did)
  const uint64_t lb = N ? S.base + sp_bend(A, N - 1u) : ci.bend;
  const int64_t lr = N ? A.rend[N - 1u] : ci.rend;
  if (open_in && n_sen != 0u && S.sen_cap != 0u) { S.sen_bstart[0] = ci.bstart; S.sen_rstart[0] = ci.rstart; }
  if (!still && n_sen != 0u && n_sen - 1u < S.sen_cap) {  // a call behind the last token, or the stream's end, closes the last row
    S.sen_tok_end[n_sen - 1u] = N;
    S.sen_bend[n_sen - 1u] = lb;
    S.sen_rend[n_sen - 1u] = lr;
  }
  DtkSenCarry co{};
  if (still) {
    co.open = 1u;
    co.bend = lb;
    co.rend = lr;
    if (firsts == 0u) { co.bstart = ci.bstart; co.rstart = ci.rstart; }  // (else k_ss_write: the row's first token)
  }
  T.carry_in = ci;
  T.carry_out = co;
  *S.trailer = T;
  *S.carry_out = co;
}

// ---------------------------------------------------------------- the rows
__global__ __launch_bounds__(256) void k_ss_write(SArgs S) {
  const Args &A = S.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t k = blockIdx.x * SP_THREADS + threadIdx.x;
  if (k >= N || !(A.tok_meta[k] >> 31)) return;
  const uint64_t open_in = S.trailer->carry_in.open ? 1u : 0u;
  const uint64_t i = open_in + ss_firsts_before(S, k);
  const uint64_t bs = S.base + A.tok_bstart[k];
  const int64_t rs = A.rstart[k];
  if (i < S.trailer->n_sen) {
    if (i < S.sen_cap) { S.sen_bstart[i] = bs; S.sen_rstart[i] = rs; }
  } else {  // the row that is open behind the slice (behind k_ss_scan's stores of the two blocks)
    S.carry_out->bstart = bs; S.carry_out->rstart = rs;
    S.trailer->carry_out.bstart = bs; S.trailer->carry_out.rstart = rs;
  }
  if (i != 0u && i - 1u < S.sen_cap) {  // the calls in front of this token closed the row before
    S.sen_tok_end[i - 1u] = k;
    S.sen_bend[i - 1u] = k ? S.base + sp_bend(A, k - 1u) : S.trailer->carry_in.bend;
    S.sen_rend[i - 1u] = k ? A.rend[k - 1u] : S.trailer->carry_in.rend;
  }
}

// ---------------------------------------------------------------- the text rows
__global__ __launch_bounds__(256) void k_ss_text(SArgs S) {
  const Args &A = S.front;
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t N = (uint32_t)A.n_tok;
  const uint32_t g = blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= A.hdr->n_te || g >= S.text_cap) return;
  const uint32_t tl = lower_bound32(A.tok_bend, N, A.evl_pos[A.te_idx[g]]);  // (as k_so_text: the tokens in front of the TextEnd)
  S.text_sen_end[g] = (uint32_t)((S.trailer->carry_in.open ? 1u : 0u) + ss_firsts_before(S, tl));
}

}  // namespace

// Lays the unit's own workspace out in `ws` (64-bit words; null: only the size is wanted) and returns its words.
extern "C" uint64_t dtk_streamsens_ws(struct DtkStreamSensArgs *s, uint64_t *ws) {
  const uint64_t N = s->front.n_tok, tt = s->front.tok_tiles;
  uint64_t at = 0;
  auto take = [&](uint64_t words) { uint64_t *p = ws ? ws + at : nullptr; at += words; return p; };
  s->first_base = take(tt);
  s->first_mask = take((N + WAVE - 1u) / WAVE);
  return at;
}

// events: null, or DTK_STREAMSENS_EVENTS events that are recorded in front of the first launch and behind each of the
// four (a launch that is left out records too): the per-launch times of scripts/stream_sentences.py.
extern "C" int dtk_launch_streamsens(const DtkStreamSensArgs *args, void *stream, void **events) {
  SArgs S = *args;
  const Args &A = S.front;
  hipStream_t s = (hipStream_t)stream;
  if (A.n_tok >= 0x80000000ull || A.tok_tiles != dtk_streamrender_tiles(A.n_tok) ||
      A.ent_tiles != dtk_streamrender_tiles(A.evl_cap) || !A.hdr || !A.carry_out || !S.carry_in || !S.carry_out ||
      S.carry_in == S.carry_out || !S.trailer || !S.text_sen_end || !S.text_cap ||
      (A.n_tok && (!A.rstart || !A.rend || !A.tok_meta || !S.first_base || !S.first_mask)) ||
      (S.sen_cap && (!S.sen_tok_end || !S.sen_bstart || !S.sen_bend || !S.sen_rstart || !S.sen_rend)))
    return 1;
  const dim3 tb(SP_THREADS);
  uint32_t n_marks = 0;
  auto mark = [&] {
    if (events && n_marks < DTK_STREAMSENS_EVENTS) (void)hipEventRecord((hipEvent_t)events[n_marks], s);
    n_marks++;
  };
  mark();
  if (A.tok_tiles) hipLaunchKernelGGL(k_ss_count, dim3(A.tok_tiles), tb, 0, s, S);
  mark();
  hipLaunchKernelGGL(k_ss_scan, dim3(1), tb, 0, s, S);
  mark();
  if (A.tok_tiles) hipLaunchKernelGGL(k_ss_write, dim3(A.tok_tiles), tb, 0, s, S);
  mark();
  if (A.ent_tiles) hipLaunchKernelGGL(k_ss_text, dim3(A.ent_tiles), tb, 0, s, S);
  mark();
  return (int)hipGetLastError();
}
