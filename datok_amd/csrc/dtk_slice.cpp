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

// What a first copy brings of a piece whose length only the trailer knows: `bound`, from the compaction's counts for
// the window as a fresh document (the delivery brings the rest if the trailer counts more), or the debug key EVL_CAP,
// so that ordinary text gets there.
uint64_t first_copy(uint64_t bound) { return g_dbg.evl_cap >= 0 ? (uint64_t)g_dbg.evl_cap : bound; }

// At delivery: what has been asked for beyond the first copies comes now, with one wait for all of it.  The kernels'
// results stay where they are on the device, nothing is computed again.
int bring_late(dtk_batch *b, MirrorBlock &m) {
  const int rc = m.issue(b->dl_stream);
  if (rc != DTK_OK || !m.in_flight) return rc;
  HIP_TRY(hipStreamSynchronize(b->dl_stream));
  m.landed();
  return DTK_OK;
}

// kPlainBytes.  The output is sized here: a surface byte per window byte of the slice (three where the run saw invalid
// UTF-8), a newline per token, SentenceEnd and TextEnd call, and the tail's two.
int render_slice(dtk_batch *b) {
  SliceOut &o = b->slice;
  SliceOut::Bytes &B = o.bytes;
  const uint64_t span = o.req.cut > o.req.first ? o.req.cut - o.req.first : 0;
  const uint64_t cap = span * (b->n_invalid ? 3u : 1u) + b->totals.n_tokens + b->totals.n_sent + b->totals.n_texts + 2;
  DtkStreamRenderArgs a{};
  a.bits = o.req.bits & 3u;
  set_slice_inputs(b, a);
  const uint64_t words = (uint64_t)a.tok_tiles + a.ent_tiles + a.evl_cap + 1;
  B.clear(); B.add(B.out, cap); B.add(B.len, 1);
  int rc;
  if ((rc = B.fit()) || (rc = o.d_ws.fit(words, words + words / 8 + 16))) return rc;
  a.tok_base = o.d_ws; a.ent_base = a.tok_base + a.tok_tiles; a.ew = a.ent_base + a.ent_tiles;
  a.out = B.dev(B.out); a.cap = cap; a.out_len = B.dev(B.len);
  HIP_TRY(hipMemsetAsync(a.out, '\n', B.at(B.len), b->dl_stream));  // every byte that is no surface byte
  if (dtk_launch_streamrender(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "render slice");
  B.bring(B.out, cap); B.bring(B.len, 1);
  return B.issue(b->dl_stream);
}

// kPosBytes.  The capacity is a bound the host can state before anything is enqueued: the
// kernels render nothing for a list of more than `rows` entries, so the slice has at most 2 * rows + 1 SentenceEnd
// calls and rows + 1 TextEnd calls; a token pushes two position integers, and a sentence integer comes from a token
// behind such a call or from a SentenceEnd call; no integer has more than `digits` bytes.  The open fragments lie behind
// the output inside the same bound.
int render_slice_pos(dtk_batch *b) {
  SliceOut &o = b->slice;
  SliceOut::Bytes &B = o.bytes;
  const SliceRequest &q = o.req;
  if (!q.carry_in || !q.carry_out) return DTK_E_STATE;
  const uint64_t span = q.cut > q.first ? q.cut - q.first : 0;
  const uint64_t rows = b->evl_copied, nt = b->totals.n_tokens;
  const uint64_t calls = 3 * rows + 2;
  const uint64_t ints = ((q.bits & DTK_TOKEN_POS) ? 2 * nt : 0) +
                        ((q.bits & DTK_SENTENCE_POS) ? std::min<uint64_t>(nt, calls + 1) + 2 * rows + 1 : 0);
  const uint64_t cap = ((q.bits & DTK_TOKENS) ? span * (b->n_invalid ? 3u : 1u) + nt : 0) + calls +
                       ints * ((uint64_t)q.digits + 1u) + 2 * (rows + 2);
  DtkStreamPosArgs a{};
  a.bits = q.bits & 31u;
  set_slice_inputs(b, a);
  const uint64_t words = dtk_streampos_ws(&a, nullptr);
  B.clear(); B.add(B.out, cap); B.add(B.trailer, 1);
  int rc;
  if ((rc = B.fit()) || (rc = o.d_ws.fit(words, words + words / 8 + 16))) return rc;
  (void)dtk_streampos_ws(&a, o.d_ws);
  a.out = B.dev(B.out); a.cap = cap; a.trailer = B.dev(B.trailer);
  HIP_TRY(hipMemsetAsync(a.out, '\n', B.at(B.trailer), b->dl_stream));  // every byte that is no surface byte and no integer's
  if (dtk_launch_streampos(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "render slice positions");
  B.bring(B.out, cap); B.bring(B.trailer, 1);
  return B.issue(b->dl_stream);
}

// offs.  The capacities are bounds the host can state before anything is enqueued, from the
// tokens and the list's rows: the kernels compute nothing for a list of more than `rows` entries, so the slice has at
// most 2 * rows + 1 SentenceEnd calls and rows + 1 TextEnd calls; a SentenceEnd call pushes one int, and a token pushes
// one if such a call (or the carry) lies in front of it.  Without offs (the sentence rows alone want the chain's device
// results) the form is the plain one and nothing is copied home.  *chain: the chain's arguments as they were launched.
int slice_offsets(dtk_batch *b, DtkStreamOffsArgs *chain) {
  SliceOut &o = b->slice;
  SliceOut::Offs &L = o.offs;
  const SliceRequest &q = o.req;
  if (!q.carry_in || !q.carry_out) return DTK_E_STATE;
  const uint64_t rows = b->evl_copied, nt = b->totals.n_tokens;
  L.blocked = q.offs && q.form == DTK_SO_BLOCKED;
  L.clear();
  L.add(L.rstart, nt); L.add(L.rend, nt); L.add(L.sent, std::min<uint64_t>(nt, 3 * rows + 3) + 2 * rows + 1);
  L.add(L.trailer, 1); L.add(L.ttok, rows + 1); L.add(L.tsent, rows + 1);
  L.add(L.heads, L.blocked ? blocks_of(nt) : 0); L.add(L.words, L.blocked ? nt : 0);
  DtkStreamOffsArgs a{};
  DtkStreamPosArgs &f = a.front;
  f.bits = DTK_TOKEN_POS | DTK_SENTENCE_POS | (q.nl ? (uint32_t)DTK_NEWLINE_AFTER_EOT : 0u);
  set_slice_inputs(b, f);
  const uint64_t words = dtk_streamoffs_ws(&a, nullptr);
  int rc;
  if ((rc = o.d_offs_ws.fit(words, words + words / 8 + 16)) || (rc = L.fit(q.offs))) return rc;
  (void)dtk_streamoffs_ws(&a, o.d_offs_ws);
  f.rstart = L.dev(L.rstart); f.rend = L.dev(L.rend);
  a.sent = L.dev(L.sent); a.sent_cap = L.cap(L.sent); a.text_cap = L.cap(L.ttok);
  a.trailer = L.dev(L.trailer); a.text_tok_end = L.dev(L.ttok); a.text_sent_end = L.dev(L.tsent);
  a.blocked = L.blocked ? 1u : 0u; a.span = g_dbg.blk_span > 0 ? (uint32_t)g_dbg.blk_span : 65535u;
  a.heads = L.dev(L.heads); a.words = L.dev(L.words);
  if (dtk_launch_streamoffs(&a, b->dl_stream, nullptr)) return hip_fail(hipGetLastError(), "slice offsets");
  *chain = a;
  if (!q.offs) return DTK_OK;
  // the plain or the blocked offsets whole; sent and the text rows as far as the compaction's counts reach (they differ
  // from the stream's by the few calls in front of the slice's first token); the trailer
  if (!L.blocked) { L.bring(L.rstart, nt); L.bring(L.rend, nt); }
  L.bring(L.sent, first_copy(b->totals.n_sent + 64));
  L.bring(L.trailer, 1);
  L.bring(L.ttok, first_copy(b->totals.n_texts + 2)); L.bring(L.tsent, first_copy(b->totals.n_texts + 2));
  L.bring(L.heads, L.cap(L.heads)); L.bring(L.words, L.cap(L.words));
  return L.issue(b->dl_stream);
}

// sens, behind the offsets chain `chain` of the same slice.  A sentence-first token needs a call or the carry in front
// of it, and the carried row is one more: min(n_tok, 3 * rows + 3) + 1 rows, and a text row per TextEnd as above.
int slice_sentences(dtk_batch *b, const DtkStreamOffsArgs &chain) {
  SliceOut &o = b->slice;
  SliceOut::Sens &L = o.sens;
  const SliceRequest &q = o.req;
  if (!q.sen_carry_in || !q.sen_carry_out) return DTK_E_STATE;
  const uint64_t rows = b->evl_copied, nt = b->totals.n_tokens, sen_cap = std::min<uint64_t>(nt, 3 * rows + 3) + 1;
  L.n = nt;
  L.clear();
  L.add(L.trailer, 1); L.add(L.tse, rows + 1);
  L.add(L.tok_end, sen_cap); L.add(L.bstart, sen_cap); L.add(L.bend, sen_cap); L.add(L.rstart, sen_cap); L.add(L.rend, sen_cap);
  DtkStreamSensArgs a{};
  a.front = chain.front;
  a.base = q.base; a.carry_in = q.sen_carry_in; a.carry_out = q.sen_carry_out;
  const uint64_t words = dtk_streamsens_ws(&a, nullptr);
  int rc;
  if ((rc = o.d_sens_ws.fit(words + 1u, words + words / 8 + 16)) || (rc = L.fit())) return rc;
  (void)dtk_streamsens_ws(&a, o.d_sens_ws);
  a.sen_cap = sen_cap; a.text_cap = L.cap(L.tse);
  a.trailer = L.dev(L.trailer); a.text_sen_end = L.dev(L.tse); a.sen_tok_end = L.dev(L.tok_end);
  a.sen_bstart = L.dev(L.bstart); a.sen_bend = L.dev(L.bend); a.sen_rstart = L.dev(L.rstart); a.sen_rend = L.dev(L.rend);
  if (dtk_launch_streamsens(&a, b->dl_stream, nullptr)) return hip_fail(hipGetLastError(), "slice sentences");
  // What the copies bring of the rows, from the compaction's counts for the window as a fresh document: there every row
  // pushes one sent int with its first token, and a second one unless a TextEnd or the window's end closes it, so
  // 2 * rows <= n_sent + n_texts + 1 (half of n_sent + 64 rows' bytes on running text; the carried row and the calls in
  // front of the first token are inside the 64).
  const uint64_t sen_home = first_copy((b->totals.n_sent + b->totals.n_texts + 1) / 2 + 64);
  L.bring(L.trailer, 1); L.bring(L.tse, first_copy(b->totals.n_texts + 2));
  L.bring(L.tok_end, sen_home); L.bring(L.bstart, sen_home); L.bring(L.bend, sen_home); L.bring(L.rstart, sen_home); L.bring(L.rend, sen_home);
  return L.issue(b->dl_stream);
}

// the download that holds the slice's outputs has come home
bool slice_home(const dtk_batch *b) { return b->dl_begun && b->dl_waited; }
}  // namespace

int slice_outputs(dtk_batch *b) {
  SliceOut &o = b->slice;
  const SliceRequest &q = o.req;
  if (q.bytes == SliceRequest::kNoBytes && !q.offs && !q.sens) return DTK_OK;
  if (b->n_docs != 1 || b->total > 0xFFFFFFFFull) return DTK_E_STATE;
  int rc = DTK_OK;
  if (q.bytes != SliceRequest::kNoBytes) rc = q.bytes == SliceRequest::kPosBytes ? render_slice_pos(b) : render_slice(b);
  DtkStreamOffsArgs chain{};  // (once per slice, whoever wants it)
  if (rc == DTK_OK && (q.offs || q.sens)) rc = slice_offsets(b, &chain);
  if (rc == DTK_OK && q.sens) rc = slice_sentences(b, chain);
  // (the download's event lies behind these copies, and nothing is handed out before it has been waited for: slice_home)
  o.bytes.landed(); o.offs.landed(); o.sens.landed();
  return rc;
}

int batch_render_out(dtk_batch *b, const uint8_t **out, uint64_t *out_len) {
  const SliceOut::Bytes &B = b->slice.bytes;
  if (b->slice.req.bytes != SliceRequest::kPlainBytes || !slice_home(b) || !B.h.p) return DTK_E_STATE;
  const uint64_t n = *B.host(B.len);
  if (n > B.cap(B.out)) return DTK_E_CAPACITY;  // (more calls than the totals count: no regular slice)
  *out = B.host(B.out);
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
  const SliceOut::Bytes &B = b->slice.bytes;
  if (b->slice.req.bytes != SliceRequest::kPosBytes || !slice_home(b) || !B.h.p) return DTK_E_STATE;
  const DtkPosTrailer *t = B.host(B.trailer);
  const int rc = dtk_pos_trailer_check(t, B.cap(B.out));
  if (rc != DTK_OK) return rc;
  *out = B.host(B.out);
  *trailer = t;
  return DTK_OK;
}

int batch_offs_out(dtk_batch *b, SoView *v) {
  SliceOut::Offs &L = b->slice.offs;
  if (!b->slice.req.offs || !slice_home(b) || !L.h.p) return DTK_E_STATE;
  const DtkOffsTrailer *t = L.host(L.trailer);
  // (a list longer than its arrays says so with n_tok = ~0; more calls than the bound counts: no regular slice)
  if (t->n_tok != L.cap(L.rstart) || t->n_sent > L.cap(L.sent) || t->n_text > L.cap(L.ttok)) return DTK_E_CAPACITY;
  if (t->flags & 1u) return DTK_E_IRREGULAR;
  // The slow paths, as a list that is packed again: a segment of a block spans more than 16 bits, so the plain arrays
  // come over now; the slice has more sent ints or text rows than the copies brought.
  const bool plain = !L.blocked || t->blk_fail;
  if (plain) { L.bring(L.rstart, t->n_tok); L.bring(L.rend, t->n_tok); }
  L.bring(L.sent, t->n_sent); L.bring(L.ttok, t->n_text); L.bring(L.tsent, t->n_text);
  const int rc = bring_late(b, L);
  if (rc != DTK_OK) return rc;
  v->t = t;
  v->rstart = plain ? L.host(L.rstart) : nullptr; v->rend = plain ? L.host(L.rend) : nullptr;
  v->words = plain ? nullptr : L.host(L.words); v->heads = plain ? nullptr : L.host(L.heads);
  v->sent = L.host(L.sent); v->ttok = L.host(L.ttok); v->tsent = L.host(L.tsent);
  return DTK_OK;
}

int batch_sens_out(dtk_batch *b, SsView *v) {
  SliceOut::Sens &L = b->slice.sens;
  if (!b->slice.req.sens || !slice_home(b) || !L.h.p) return DTK_E_STATE;
  const DtkSensTrailer *t = L.host(L.trailer);
  // (a list longer than its arrays says so with n_tok = ~0; more rows than the bound counts: no regular slice)
  if (t->n_tok != L.n || t->n_sen > L.cap(L.tok_end) || t->n_text > L.cap(L.tse) || t->firsts > L.n) return DTK_E_CAPACITY;
  if (t->flags & 1u) return DTK_E_IRREGULAR;
  // the slice closed more rows or texts than the copies brought
  L.bring(L.tok_end, t->n_sen); L.bring(L.bstart, t->n_sen); L.bring(L.bend, t->n_sen); L.bring(L.rstart, t->n_sen); L.bring(L.rend, t->n_sen);
  L.bring(L.tse, t->n_text);
  const int rc = bring_late(b, L);
  if (rc != DTK_OK) return rc;
  v->t = t;
  v->tok_end = L.host(L.tok_end); v->tse = L.host(L.tse);
  v->bstart = L.host(L.bstart); v->bend = L.host(L.bend); v->rstart = L.host(L.rstart); v->rend = L.host(L.rend);
  return DTK_OK;
}
