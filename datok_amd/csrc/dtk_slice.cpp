// dtk_slice.cpp -- what a slice of a stream brings home beside its batch's result arrays (SliceRequest, dtk_host.h): the
// writer's bytes in a position-free mode or in a position mode, the writer's rune offsets and sentence list as
// arrays, and the sentences as rows.  All of it is computed on the download stream behind the list's kernels and in front of the copies
// (slice_outputs, called by dtk_batch_download_begin behind every packing of the event list), into buffers that are
// sized from what the host knows before anything is enqueued, and handed out behind dtk_batch_result_host.
#include <algorithm>
#include <type_traits>

#include "dtk_host.h"

namespace {
// The inputs the kernels' argument blocks share -- the window, the tokens, the event list (`rows`: what its arrays hold
// and the copies bring), the tail word, the tiles --, into the fields of the same names of `a` (DtkStreamRenderArgs or
// DtkStreamPosArgs).  A position block also gets where the calls begin and the carry slots.
template <class A>
void set_slice_inputs(const dtk_batch *b, A &a) {
  const SliceRequest &q = b->slice.req;
  a.with_tail = q.last ? 1u : 0u;
  a.text = b->d_text; a.text_len = (uint32_t)b->total;
  a.sym = sym_of(b); if (!b->n_invalid) a.sym.base = nullptr;
  a.n_tok = b->totals.n_tokens; a.tok_bstart = b->d_bstart; a.tok_bend = b->d_bend;
  a.evl_pos = b->d_evl_pos; a.evl_kind = b->d_evl_kind; a.evl_count = b->d_evl_cnt; a.evl_cap = (uint32_t)b->evl_copied;
  a.doc_tail = b->d_doc_tail;
  a.tok_tiles = dtk_streamrender_tiles(b->totals.n_tokens); a.ent_tiles = dtk_streamrender_tiles(b->evl_copied);
  if constexpr (std::is_same<A, DtkStreamPosArgs>::value) {
    a.is_matrix = q.is_matrix ? 1u : 0u; a.first = q.first;
    a.carry_in = q.carry_in; a.carry_out = q.carry_out;
  }
}

// kPlainBytes.  The output is sized here: a surface byte per window byte of the slice (three where the run saw invalid
// UTF-8), a newline per token, SentenceEnd and TextEnd call, and the tail's two.
int render_slice(dtk_batch *b) {
  SliceOut &o = b->slice;
  const uint64_t span = o.req.cut > o.req.first ? o.req.cut - o.req.first : 0;
  const uint64_t cap = span * (b->n_invalid ? 3u : 1u) + b->totals.n_tokens + b->totals.n_sent + b->totals.n_texts + 2;
  const uint64_t cap8 = (cap + 7u) & ~7ull;  // (the length word lies behind the bytes)
  DtkStreamRenderArgs a{};
  a.bits = o.req.bits & 3u;
  set_slice_inputs(b, a);
  const uint64_t words = (uint64_t)a.tok_tiles + a.ent_tiles + a.evl_cap + 1;
  int rc;
  if ((rc = o.d_out.fit(cap8 + 8, cap8 + cap8 / 8 + 264)) || (rc = o.d_ws.fit(words, words + words / 8 + 16)) ||
      (rc = o.h_out.fit((size_t)(cap8 + 8))))
    return rc;
  a.tok_base = o.d_ws; a.ent_base = a.tok_base + a.tok_tiles; a.ew = a.ent_base + a.ent_tiles;
  a.out = o.d_out; a.cap = cap; a.out_len = reinterpret_cast<uint64_t *>(o.d_out.p + cap8);
  HIP_TRY(hipMemsetAsync(o.d_out, '\n', cap8, b->dl_stream));  // every byte that is no surface byte
  if (dtk_launch_streamrender(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "render slice");
  HIP_TRY(hipMemcpyAsync(o.h_out.p, o.d_out, (size_t)(cap8 + 8), hipMemcpyDeviceToHost, b->dl_stream));
  o.cap = cap;
  return DTK_OK;
}

// kPosBytes.  The capacity is a bound the host can state before anything is enqueued: the
// kernels render nothing for a list of more than `rows` entries, so the slice has at most 2 * rows + 1 SentenceEnd
// calls and rows + 1 TextEnd calls; a token pushes two position integers, and a sentence integer comes from a token
// behind such a call or from a SentenceEnd call; no integer has more than `digits` bytes.  The open fragments lie behind
// the output inside the same bound.
int render_slice_pos(dtk_batch *b) {
  SliceOut &o = b->slice;
  const SliceRequest &q = o.req;
  if (!q.carry_in || !q.carry_out) return DTK_E_STATE;
  const uint64_t span = q.cut > q.first ? q.cut - q.first : 0;
  const uint64_t rows = b->evl_copied, nt = b->totals.n_tokens;
  const uint64_t calls = 3 * rows + 2;
  const uint64_t ints = ((q.bits & DTK_TOKEN_POS) ? 2 * nt : 0) +
                        ((q.bits & DTK_SENTENCE_POS) ? std::min<uint64_t>(nt, calls + 1) + 2 * rows + 1 : 0);
  const uint64_t cap = ((q.bits & DTK_TOKENS) ? span * (b->n_invalid ? 3u : 1u) + nt : 0) + calls +
                       ints * ((uint64_t)q.digits + 1u) + 2 * (rows + 2);
  const uint64_t cap8 = (cap + 7u) & ~7ull;
  const uint64_t bytes = cap8 + sizeof(DtkPosTrailer);
  DtkStreamPosArgs a{};
  a.bits = q.bits & 31u;
  set_slice_inputs(b, a);
  const uint64_t words = dtk_streampos_ws(&a, nullptr);
  int rc;
  if ((rc = o.d_out.fit(bytes, bytes + bytes / 8 + 264)) || (rc = o.d_ws.fit(words, words + words / 8 + 16)) ||
      (rc = o.h_out.fit((size_t)bytes)))
    return rc;
  (void)dtk_streampos_ws(&a, o.d_ws);
  a.out = o.d_out; a.cap = cap; a.trailer = reinterpret_cast<DtkPosTrailer *>(o.d_out.p + cap8);
  HIP_TRY(hipMemsetAsync(o.d_out, '\n', cap8, b->dl_stream));  // every byte that is no surface byte and no integer's
  if (dtk_launch_streampos(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "render slice positions");
  HIP_TRY(hipMemcpyAsync(o.h_out.p, o.d_out, (size_t)bytes, hipMemcpyDeviceToHost, b->dl_stream));
  o.cap = cap;
  return DTK_OK;
}

// offs.  The capacities are bounds the host can state before anything is enqueued, from the
// tokens and the list's rows: the kernels compute nothing for a list of more than `rows` entries, so the slice has at
// most 2 * rows + 1 SentenceEnd calls and rows + 1 TextEnd calls; a SentenceEnd call pushes one int, and a token pushes
// one if such a call (or the carry) lies in front of it.  Without offs (the sentence rows alone want the chain's device
// results) the form is the plain one and nothing is copied home.  *chain: the chain's arguments as they were launched.
int slice_offsets(dtk_batch *b, DtkStreamOffsArgs *chain) {
  SliceOut &o = b->slice;
  const SliceRequest &q = o.req;
  if (!q.carry_in || !q.carry_out) return DTK_E_STATE;
  const uint64_t rows = b->evl_copied, nt = b->totals.n_tokens;
  SoLayout L;
  L.n = nt; L.sent_cap = std::min<uint64_t>(nt, 3 * rows + 3) + 2 * rows + 1; L.text_cap = rows + 1;
  L.blocked = q.offs && q.form == DTK_SO_BLOCKED;
  // What the copies bring of sent and the text rows: the compaction's counts for the window as a fresh document, which
  // differ from the stream's by the few calls in front of the slice's first token.  batch_offs_out brings the rest if
  // the trailer counts more (the debug key EVL_CAP sizes these too, so that ordinary text gets there).
  L.sent_home = std::min<uint64_t>(L.sent_cap, g_dbg.evl_cap >= 0 ? (uint64_t)g_dbg.evl_cap : b->totals.n_sent + 64);
  L.text_home = std::min<uint64_t>(L.text_cap, g_dbg.evl_cap >= 0 ? (uint64_t)g_dbg.evl_cap : b->totals.n_texts + 2);
  uint64_t at = 0;  // (bytes; every piece begins on a multiple of 8)
  auto take = [&](uint64_t bytes) { const uint64_t p = at; at += (bytes + 7u) & ~7ull; return p; };
  L.rstart = take(nt * 8); L.rend = take(nt * 8); L.sent = take(L.sent_cap * 8);
  L.trailer = take(sizeof(DtkOffsTrailer)); L.ttok = take(L.text_cap * 4); L.tsent = take(L.text_cap * 4);
  L.heads = take(L.blocked ? blocks_of(nt) * sizeof(DtkOffBlock64) : 0); L.words = take(L.blocked ? nt * 4 : 0);
  L.bytes = at;
  DtkStreamOffsArgs a{};
  DtkStreamPosArgs &f = a.front;
  f.bits = DTK_TOKEN_POS | DTK_SENTENCE_POS | (q.nl ? (uint32_t)DTK_NEWLINE_AFTER_EOT : 0u);
  set_slice_inputs(b, f);
  const uint64_t words = dtk_streamoffs_ws(&a, nullptr), out_words = L.bytes / 8;
  int rc;
  if ((rc = o.d_offs_ws.fit(words, words + words / 8 + 16)) || (rc = o.d_offs_out.fit(out_words, out_words + out_words / 8 + 32)) ||
      (q.offs && (rc = o.h_offs_out.fit((size_t)L.bytes))))
    return rc;
  (void)dtk_streamoffs_ws(&a, o.d_offs_ws);
  uint8_t *d = reinterpret_cast<uint8_t *>(o.d_offs_out.p), *h = o.h_offs_out.as<uint8_t>();
  f.rstart = reinterpret_cast<int64_t *>(d + L.rstart); f.rend = reinterpret_cast<int64_t *>(d + L.rend);
  a.sent = reinterpret_cast<int64_t *>(d + L.sent); a.sent_cap = L.sent_cap; a.text_cap = L.text_cap;
  a.trailer = reinterpret_cast<DtkOffsTrailer *>(d + L.trailer);
  a.text_tok_end = reinterpret_cast<uint32_t *>(d + L.ttok); a.text_sent_end = reinterpret_cast<uint32_t *>(d + L.tsent);
  a.blocked = L.blocked ? 1u : 0u; a.span = g_dbg.blk_span > 0 ? (uint32_t)g_dbg.blk_span : 65535u;
  a.heads = reinterpret_cast<DtkOffBlock64 *>(d + L.heads); a.words = reinterpret_cast<uint32_t *>(d + L.words);
  if (dtk_launch_streamoffs(&a, b->dl_stream, nullptr)) return hip_fail(hipGetLastError(), "slice offsets");
  *chain = a;
  o.so = L;
  if (!q.offs) return DTK_OK;
  // the plain offsets and sent lie back to back; then the trailer with text_tok_end, text_sent_end, the blocked form
  const uint64_t piece[4][2] = {{L.blocked ? L.sent : 0, L.sent + L.sent_home * 8},
                                {L.trailer, L.ttok + L.text_home * 4},
                                {L.tsent, L.tsent + L.text_home * 4},
                                {L.heads, L.blocked ? L.bytes : L.heads}};
  for (const auto &p : piece)
    if (p[1] > p[0]) HIP_TRY(hipMemcpyAsync(h + p[0], d + p[0], (size_t)(p[1] - p[0]), hipMemcpyDeviceToHost, b->dl_stream));
  o.so.wide_home = !L.blocked;
  return DTK_OK;
}

// sens, behind the offsets chain `chain` of the same slice.  A sentence-first token needs a call or the carry in front
// of it, and the carried row is one more: min(n_tok, 3 * rows + 3) + 1 rows, and a text row per TextEnd as above.
int slice_sentences(dtk_batch *b, const DtkStreamOffsArgs &chain) {
  SliceOut &o = b->slice;
  const SliceRequest &q = o.req;
  if (!q.sen_carry_in || !q.sen_carry_out) return DTK_E_STATE;
  const uint64_t rows = b->evl_copied, nt = b->totals.n_tokens;
  SsLayout L;
  L.n = nt; L.sen_cap = std::min<uint64_t>(nt, 3 * rows + 3) + 1; L.text_cap = rows + 1;
  // What the copies bring of the rows, from the compaction's counts for the window as a fresh document: there every row
  // pushes one sent int with its first token, and a second one unless a TextEnd or the window's end closes it, so
  // 2 * rows <= n_sent + n_texts + 1 (half of n_sent + 64 rows' bytes on running text; the carried row and the calls in
  // front of the first token are inside the 64).  batch_sens_out brings the rest if the trailer counts more.
  L.sen_home = std::min<uint64_t>(L.sen_cap, g_dbg.evl_cap >= 0 ? (uint64_t)g_dbg.evl_cap
                                                                : (b->totals.n_sent + b->totals.n_texts + 1) / 2 + 64);
  L.text_home = std::min<uint64_t>(L.text_cap, g_dbg.evl_cap >= 0 ? (uint64_t)g_dbg.evl_cap : b->totals.n_texts + 2);
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) { const uint64_t p = at; at += (bytes + 7u) & ~7ull; return p; };
  L.trailer = take(sizeof(DtkSensTrailer)); L.tse = take(L.text_cap * 4);
  L.tok_end = take(L.sen_cap * 4); L.bstart = take(L.sen_cap * 8); L.bend = take(L.sen_cap * 8);
  L.rstart = take(L.sen_cap * 8); L.rend = take(L.sen_cap * 8);
  L.bytes = at;
  DtkStreamSensArgs a{};
  a.front = chain.front;
  a.base = q.base; a.carry_in = q.sen_carry_in; a.carry_out = q.sen_carry_out;
  const uint64_t words = dtk_streamsens_ws(&a, nullptr), out_words = L.bytes / 8;
  int rc;
  if ((rc = o.d_sens_ws.fit(words + 1u, words + words / 8 + 16)) || (rc = o.d_sens_out.fit(out_words, out_words + out_words / 8 + 32)) ||
      (rc = o.h_sens_out.fit((size_t)L.bytes)))
    return rc;
  (void)dtk_streamsens_ws(&a, o.d_sens_ws);
  uint8_t *d = reinterpret_cast<uint8_t *>(o.d_sens_out.p), *h = o.h_sens_out.as<uint8_t>();
  a.sen_cap = L.sen_cap; a.text_cap = L.text_cap;
  a.trailer = reinterpret_cast<DtkSensTrailer *>(d + L.trailer);
  a.text_sen_end = reinterpret_cast<uint32_t *>(d + L.tse);
  a.sen_tok_end = reinterpret_cast<uint32_t *>(d + L.tok_end);
  a.sen_bstart = reinterpret_cast<uint64_t *>(d + L.bstart); a.sen_bend = reinterpret_cast<uint64_t *>(d + L.bend);
  a.sen_rstart = reinterpret_cast<int64_t *>(d + L.rstart); a.sen_rend = reinterpret_cast<int64_t *>(d + L.rend);
  if (dtk_launch_streamsens(&a, b->dl_stream, nullptr)) return hip_fail(hipGetLastError(), "slice sentences");
  // the trailer with text_sen_end behind it, then the five arrays
  const uint64_t piece[6][2] = {{L.trailer, L.tse + L.text_home * 4},       {L.tok_end, L.tok_end + L.sen_home * 4},
                                {L.bstart, L.bstart + L.sen_home * 8},      {L.bend, L.bend + L.sen_home * 8},
                                {L.rstart, L.rstart + L.sen_home * 8},      {L.rend, L.rend + L.sen_home * 8}};
  for (const auto &p : piece)
    if (p[1] > p[0]) HIP_TRY(hipMemcpyAsync(h + p[0], d + p[0], (size_t)(p[1] - p[0]), hipMemcpyDeviceToHost, b->dl_stream));
  o.ss = L;
  return DTK_OK;
}

// the download that holds the slice's outputs has come home
bool slice_home(const dtk_batch *b) { return b->dl_begun && b->dl_waited; }
}  // namespace

int slice_outputs(dtk_batch *b) {
  const SliceRequest &q = b->slice.req;
  if (q.bytes == SliceRequest::kNoBytes && !q.offs && !q.sens) return DTK_OK;
  if (b->n_docs != 1 || b->total > 0xFFFFFFFFull) return DTK_E_STATE;
  int rc = DTK_OK;
  if (q.bytes != SliceRequest::kNoBytes) rc = q.bytes == SliceRequest::kPosBytes ? render_slice_pos(b) : render_slice(b);
  DtkStreamOffsArgs chain{};  // (once per slice, whoever wants it)
  if (rc == DTK_OK && (q.offs || q.sens)) rc = slice_offsets(b, &chain);
  if (rc == DTK_OK && q.sens) rc = slice_sentences(b, chain);
  return rc;
}

int batch_render_out(dtk_batch *b, const uint8_t **out, uint64_t *out_len) {
  const SliceOut &o = b->slice;
  if (o.req.bytes != SliceRequest::kPlainBytes || !slice_home(b) || !o.h_out.p) return DTK_E_STATE;
  const uint64_t cap8 = (o.cap + 7u) & ~7ull;
  const uint64_t n = *reinterpret_cast<const uint64_t *>(o.h_out.as<uint8_t>() + cap8);
  if (n > o.cap) return DTK_E_CAPACITY;  // (more calls than the totals count: no regular slice)
  *out = o.h_out.as<uint8_t>();
  *out_len = n;
  return DTK_OK;
}

// What a trailer block that has come home says about its slice: never bytes that differ silently.
extern "C" int dtk_pos_trailer_check(const DtkPosTrailer *t, uint64_t cap) {
  if (!t) return DTK_E_ARG;
  // (more calls than the bound counts -- a list longer than its arrays says so with out_len = ~0 --, or a tile of
  //  tokens whose integers pass 2^32 bytes: no regular slice)
  if (t->out_len > cap || t->open_pos_len > cap || t->open_sent_len > cap ||
      t->out_len + t->open_pos_len + t->open_sent_len > cap || (t->flags & 2u))
    return DTK_E_CAPACITY;
  if (t->flags & 1u) return DTK_E_IRREGULAR;  // the newline rule would fire a second time: the exact pass's, from a carried record
  return DTK_OK;
}

int batch_pos_out(dtk_batch *b, const uint8_t **out, const DtkPosTrailer **trailer) {
  const SliceOut &o = b->slice;
  if (o.req.bytes != SliceRequest::kPosBytes || !slice_home(b) || !o.h_out.p) return DTK_E_STATE;
  const uint64_t cap8 = (o.cap + 7u) & ~7ull;
  const DtkPosTrailer *t = reinterpret_cast<const DtkPosTrailer *>(o.h_out.as<uint8_t>() + cap8);
  const int rc = dtk_pos_trailer_check(t, o.cap);
  if (rc != DTK_OK) return rc;
  *out = o.h_out.as<uint8_t>();
  *trailer = t;
  return DTK_OK;
}

int batch_offs_out(dtk_batch *b, SoView *v) {
  SliceOut &o = b->slice;
  if (!o.req.offs || !slice_home(b) || !o.h_offs_out.p) return DTK_E_STATE;
  SoLayout &L = o.so;
  const uint8_t *h = o.h_offs_out.as<uint8_t>();
  const DtkOffsTrailer *t = reinterpret_cast<const DtkOffsTrailer *>(h + L.trailer);
  // (a list longer than its arrays says so with n_tok = ~0; more calls than the bound counts: no regular slice)
  if (t->n_tok != L.n || t->n_sent > L.sent_cap || t->n_text > L.text_cap) return DTK_E_CAPACITY;
  if (t->flags & 1u) return DTK_E_IRREGULAR;
  // The slow paths, as a list that is packed again: a segment of a block spans more than 16 bits, so the plain arrays
  // come over now; the slice has more sent ints or text rows than the copies brought.  The kernels' results stay where
  // they are on the device, nothing is computed again.
  const uint8_t *d = reinterpret_cast<const uint8_t *>(o.d_offs_out.p);
  uint8_t *hw = o.h_offs_out.as<uint8_t>();
  bool late = false;
  auto bring = [&](uint64_t from, uint64_t to) -> int {
    if (to > from) HIP_TRY(hipMemcpyAsync(hw + from, d + from, (size_t)(to - from), hipMemcpyDeviceToHost, b->dl_stream));
    late = true;
    return DTK_OK;
  };
  int rc;
  if (L.blocked && t->blk_fail && !L.wide_home) {
    if ((rc = bring(0, L.sent)) != DTK_OK) return rc;
    L.wide_home = true;
  }
  if (t->n_sent > L.sent_home) {
    if ((rc = bring(L.sent + L.sent_home * 8, L.sent + t->n_sent * 8)) != DTK_OK) return rc;
    L.sent_home = t->n_sent;
  }
  if (t->n_text > L.text_home) {
    if ((rc = bring(L.ttok + L.text_home * 4, L.ttok + t->n_text * 4)) != DTK_OK ||
        (rc = bring(L.tsent + L.text_home * 4, L.tsent + t->n_text * 4)) != DTK_OK)
      return rc;
    L.text_home = t->n_text;
  }
  if (late) HIP_TRY(hipStreamSynchronize(b->dl_stream));
  const bool plain = !L.blocked || t->blk_fail;
  v->t = t;
  v->rstart = plain ? reinterpret_cast<const int64_t *>(h + L.rstart) : nullptr;
  v->rend = plain ? reinterpret_cast<const int64_t *>(h + L.rend) : nullptr;
  v->words = plain ? nullptr : reinterpret_cast<const uint32_t *>(h + L.words);
  v->heads = plain ? nullptr : reinterpret_cast<const DtkOffBlock64 *>(h + L.heads);
  v->sent = reinterpret_cast<const int64_t *>(h + L.sent);
  v->ttok = reinterpret_cast<const uint32_t *>(h + L.ttok); v->tsent = reinterpret_cast<const uint32_t *>(h + L.tsent);
  return DTK_OK;
}

int batch_sens_out(dtk_batch *b, SsView *v) {
  SliceOut &o = b->slice;
  if (!o.req.sens || !slice_home(b) || !o.h_sens_out.p) return DTK_E_STATE;
  SsLayout &L = o.ss;
  uint8_t *h = o.h_sens_out.as<uint8_t>();
  const DtkSensTrailer *t = reinterpret_cast<const DtkSensTrailer *>(h + L.trailer);
  // (a list longer than its arrays says so with n_tok = ~0; more rows than the bound counts: no regular slice)
  if (t->n_tok != L.n || t->n_sen > L.sen_cap || t->n_text > L.text_cap || t->firsts > L.n) return DTK_E_CAPACITY;
  if (t->flags & 1u) return DTK_E_IRREGULAR;
  // the slice closed more rows or texts than the copies brought: the rest comes now, nothing is computed again
  const uint8_t *d = reinterpret_cast<const uint8_t *>(o.d_sens_out.p);
  bool late = false;
  auto bring = [&](uint64_t at, uint64_t from, uint64_t to, uint64_t size) -> int {
    HIP_TRY(hipMemcpyAsync(h + at + from * size, d + at + from * size, (size_t)((to - from) * size), hipMemcpyDeviceToHost, b->dl_stream));
    late = true;
    return DTK_OK;
  };
  int rc;
  if (t->n_sen > L.sen_home) {
    if ((rc = bring(L.tok_end, L.sen_home, t->n_sen, 4)) != DTK_OK || (rc = bring(L.bstart, L.sen_home, t->n_sen, 8)) != DTK_OK ||
        (rc = bring(L.bend, L.sen_home, t->n_sen, 8)) != DTK_OK || (rc = bring(L.rstart, L.sen_home, t->n_sen, 8)) != DTK_OK ||
        (rc = bring(L.rend, L.sen_home, t->n_sen, 8)) != DTK_OK)
      return rc;
    L.sen_home = t->n_sen;
  }
  if (t->n_text > L.text_home) {
    if ((rc = bring(L.tse, L.text_home, t->n_text, 4)) != DTK_OK) return rc;
    L.text_home = t->n_text;
  }
  if (late) HIP_TRY(hipStreamSynchronize(b->dl_stream));
  v->t = t;
  v->tok_end = reinterpret_cast<const uint32_t *>(h + L.tok_end); v->tse = reinterpret_cast<const uint32_t *>(h + L.tse);
  v->bstart = reinterpret_cast<const uint64_t *>(h + L.bstart); v->bend = reinterpret_cast<const uint64_t *>(h + L.bend);
  v->rstart = reinterpret_cast<const int64_t *>(h + L.rstart); v->rend = reinterpret_cast<const int64_t *>(h + L.rend);
  return DTK_OK;
}
