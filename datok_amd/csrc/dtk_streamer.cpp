// dtk_streamer.cpp -- one stream of any length (dtk_stream_run).  The reference tokenizes whatever
// its reader delivers (bufio.Reader, matrix.go:373); here the stream is read into `depth` page-locked buffers of S + T
// bytes and walked in slices: slice k is the window [k * S, k * S + S + T) as one document of one batch, from the
// record slice k - 1 carried over, up to its cut (k_stream_cut).  Uploads, kernels and downloads of neighbouring slices
// run on three streams like a dtk_pipeline's; the walks are serialised on what the host knows: slice k is enqueued
// once slice k - 1 is finished (finish(): repairs, the EOT kernel, larger arrays included) and its cut block is home,
// so no stale record is ever fed forward.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "dtk_host.h"

namespace {
constexpr uint32_t kTail = 8192u;  // T: look-ahead behind S, so that the first sync point at or behind S (below S + DTK_WINDOW_BYTES)
                                   // and everything in front of it is walked without a sight of the window's end
static_assert(kTail >= 2u * DTK_WINDOW_BYTES - 16u && kTail % 256u == 0u, "the tail holds a window behind the latest cut");
constexpr uint32_t kForced = DTK_R_CSR | DTK_R_STATUS | DTK_R_TEXTS | DTK_R_EVENT_LIST;
}  // namespace

struct dtk_stream {
  uint64_t S = 0;
  uint32_t depth = 0;
  uint32_t fields = kForced | DTK_R_TOK_BYTE;
  // Every slice's writer bytes come with it: dtk_stream_set_render (kPlainBytes; bits: TOKENS | SENTENCES) or
  // dtk_stream_set_position_render (kPosBytes; bits: all five writer bits), one renderer at a time.
  SliceRequest::Bytes bytes = SliceRequest::kNoBytes;
  uint32_t bits = 0;
  // dtk_stream_set_offsets: the writer's rune offsets and sentence list as arrays, beside set_render's bytes or alone;
  // exclusive with position rendering.
  bool offs = false;
  uint32_t offs_form = DTK_SO_PLAIN;
  // dtk_stream_set_sentences: the sentences as rows, beside set_render's bytes, beside the offsets or alone; exclusive
  // with position rendering like the offsets.  The row that is open at a cut is chained like the writer's state, in
  // slots of its own with the same rule.
  bool sens = false;
  DevArray<DtkSenCarry> d_sen_carry;  // depth + 1
  // dtk_stream_set_vocab: the slots' batches look their tokens up (dtk_batch_set_vocab); nothing crosses a cut
  bool vocab = false;
  bool ids_home = false;
  // dtk_stream_set_wordpiece: ... and split them (dtk_batch_set_wordpiece), the same way
  bool wordpiece = false;
  bool pieces_home = false;
  // Position rendering and offset delivery follow the writer's state, which is chained on the device: slice k reads
  // carry slot k % (depth + 1) and writes the next one -- never the slot it read, and a slot is written again only by
  // slice k + depth, which takes the batch that slice k has left by then.
  DevArray<DtkPosCarry> d_carry;  // depth + 1
  // The held prefixes (dtk_stream_emit): the integers of the text that is open at the last cut, as the bytes of its
  // TOKEN_POS / SENTENCE_POS line so far.  They grow with the length of a text, as the reference's pos[] / sent[] do.
  std::string held_pos, held_sent;
  // the slice being delivered: valid inside slice_fn only
  struct Delivery {
    const uint8_t *out = nullptr;         // position rendering: the bytes, the trailer behind them (null: none),
    const DtkPosTrailer *pos = nullptr;   // and whether dtk_stream_emit has written them
    bool emitted = false;
    bool offs_set = false;                // offset delivery: offs is this slice's
    SoView offs{};
    bool sens_set = false;                // the sentence rows: sens is this slice's
    SsView sens{};
    bool ids_set = false;                 // the tokens' ids: ids is this slice's
    dtk_token_id_view ids{};
    bool pieces_set = false;              // the tokens' pieces: pieces is this slice's
    dtk_piece_view pieces{};
  } cur;
  Stream s_up, s_run, s_down;
  std::vector<dtk_batch *> slots;
  std::vector<std::unique_ptr<PinBuf>> buf;  // depth x (S + T)
  ~dtk_stream() {
    for (dtk_batch *b : slots) dtk_batch_free(b);
    for (hipStream_t st : {s_up.s, s_run.s, s_down.s})
      if (st) (void)hipStreamSynchronize(st);
  }
};

extern "C" int dtk_stream_create(uint64_t slice_bytes, uint32_t depth, dtk_stream **out) {
  if (!out) return DTK_E_ARG;
  *out = nullptr;
  if (slice_bytes < 16384u || slice_bytes % 256u != 0 || slice_bytes >= 0x7FFF0000ull || depth < 2 || depth > 16) return DTK_E_ARG;
  if (dtk_device_count() <= 0) return DTK_E_NO_DEVICE;
  std::unique_ptr<dtk_stream> s(new dtk_stream());
  s->S = slice_bytes;
  s->depth = depth;
  int rc;
  if ((rc = s->s_up.create()) || (rc = s->s_run.create()) || (rc = s->s_down.create()) ||
      (rc = s->d_carry.fit((uint64_t)depth + 1u, (uint64_t)depth + 1u)) ||
      (rc = s->d_sen_carry.fit((uint64_t)depth + 1u, (uint64_t)depth + 1u)))
    return rc;
  for (uint32_t i = 0; i < depth; i++) {
    dtk_batch *b = nullptr;
    if ((rc = dtk_batch_create(slice_bytes + kTail, 1, &b)) != DTK_OK) return rc;
    s->slots.push_back(b);
    if ((rc = dtk_batch_set_streams(b, s->s_run, s->s_up)) != DTK_OK ||
        (rc = dtk_batch_set_download_stream(b, s->s_down)) != DTK_OK ||
        (rc = dtk_batch_set_result_fields(b, s->fields)) != DTK_OK)
      return rc;
    s->buf.emplace_back(new PinBuf());
    if ((rc = s->buf.back()->fit(slice_bytes + kTail, slice_bytes + kTail)) != DTK_OK) return rc;
  }
  *out = s.release();
  return DTK_OK;
}

extern "C" void dtk_stream_free(dtk_stream *s) { delete s; }

extern "C" int dtk_stream_set_chunking(dtk_stream *s, uint32_t chunk_bytes, uint32_t warm_bytes) {
  if (!s) return DTK_E_ARG;
  // (the cut is the record of the first lane at or behind S: with chunks of up to 2048 bytes it lies below
  //  S + 2048 + DTK_WINDOW_BYTES, and the walk up to it ends in front of the window's end)
  if (chunk_bytes != 0 && chunk_bytes != 0xFFFFFFFFu && (chunk_bytes < 16 || chunk_bytes > 2048)) return DTK_E_ARG;
  for (dtk_batch *b : s->slots) {
    const int rc = dtk_batch_set_chunking(b, chunk_bytes, warm_bytes);
    if (rc != DTK_OK) return rc;
  }
  return DTK_OK;
}

extern "C" int dtk_stream_set_result_fields(dtk_stream *s, uint32_t fields) {
  if (!s || !(fields & (DTK_R_TOK_BYTE | DTK_R_TOK_BYTE_BLK))) return DTK_E_ARG;
  // (the rune fields of a slice's view would be the compaction's: the window as a fresh document.  The stream's rune
  //  offsets and sentence list come from dtk_stream_set_offsets, computed from the writer's carried state.)
  // (nor the batch's sentence table, which ends with the window: a stream's rows come from dtk_stream_set_sentences,
  //  with the open row carried across the cuts)
  if (fields & (DTK_R_TOK_RUNE | DTK_R_TOK_RUNE16 | DTK_R_TOK_RUNE_BLK | DTK_R_SENT | DTK_R_EAGER | DTK_R_SENTENCES)) return DTK_E_ARG;
  fields |= kForced;
  for (dtk_batch *b : s->slots) {
    const int rc = dtk_batch_set_result_fields(b, fields);
    if (rc != DTK_OK) return rc;
  }
  s->fields = fields;
  return DTK_OK;
}

extern "C" int dtk_stream_set_render(dtk_stream *s, int on, uint32_t bits) {
  // (the position modes keep writer state across cuts: the host writer's, through the replay)
  if (!s || (bits & ~(uint32_t)(DTK_TOKENS | DTK_SENTENCES | DTK_NEWLINE_AFTER_EOT))) return DTK_E_ARG;
  if (on) {  // (position rendering, if it was on, is off)
    s->bytes = SliceRequest::kPlainBytes;
    s->bits = bits & (uint32_t)(DTK_TOKENS | DTK_SENTENCES);
  } else if (s->bytes == SliceRequest::kPlainBytes) {
    s->bytes = SliceRequest::kNoBytes;
  }
  return DTK_OK;
}

extern "C" int dtk_stream_set_position_render(dtk_stream *s, int on, uint32_t bits) {
  const uint32_t all = DTK_TOKENS | DTK_SENTENCES | DTK_TOKEN_POS | DTK_SENTENCE_POS | DTK_NEWLINE_AFTER_EOT;
  if (!s || (bits & ~all)) return DTK_E_ARG;
  if (on && !(bits & (uint32_t)(DTK_TOKEN_POS | DTK_SENTENCE_POS))) return DTK_E_ARG;  // those modes are dtk_stream_set_render's
  if (on && (s->offs || s->sens)) return DTK_E_ARG;  // (the offsets as digits or as arrays, not both; the rows read the arrays' chain)
  if (on) {  // (plain rendering, if it was on, is off)
    s->bytes = SliceRequest::kPosBytes;
    s->bits = bits;
  } else if (s->bytes == SliceRequest::kPosBytes) {
    s->bytes = SliceRequest::kNoBytes;
  }
  return DTK_OK;
}

extern "C" int dtk_stream_set_offsets(dtk_stream *s, int on, uint32_t form) {
  if (!s) return DTK_E_ARG;
  if (on && ((form != DTK_SO_PLAIN && form != DTK_SO_BLOCKED) || s->bytes == SliceRequest::kPosBytes)) return DTK_E_ARG;
  if (on) s->offs_form = form;
  s->offs = on != 0;
  return DTK_OK;
}

extern "C" int dtk_stream_set_sentences(dtk_stream *s, int on) {
  if (!s) return DTK_E_ARG;
  if (on && s->bytes == SliceRequest::kPosBytes) return DTK_E_ARG;
  s->sens = on != 0;
  return DTK_OK;
}

extern "C" int dtk_stream_set_vocab(dtk_stream *s, const dtk_vocab *v, dtk_tally *t, int ids_home) {
  if (!s) return DTK_E_ARG;
  for (dtk_batch *b : s->slots) {
    const int rc = dtk_batch_set_vocab(b, v, t, ids_home);
    if (rc != DTK_OK) return rc;
  }
  s->vocab = v != nullptr;
  s->ids_home = v && ids_home != 0;
  return DTK_OK;
}

extern "C" int dtk_stream_token_ids(dtk_stream *s, dtk_token_id_view *o) {
  if (!s || !o) return DTK_E_ARG;
  if (!s->cur.ids_set) return DTK_E_STATE;
  *o = s->cur.ids;
  return DTK_OK;
}

extern "C" int dtk_stream_set_wordpiece(dtk_stream *s, const dtk_vocab *v, const uint8_t *prefix, uint32_t prefix_len,
                                        int32_t unk_id, uint32_t max_runes, int pieces_home) {
  if (!s) return DTK_E_ARG;
  for (dtk_batch *b : s->slots) {
    const int rc = dtk_batch_set_wordpiece(b, v, prefix, prefix_len, unk_id, max_runes, pieces_home);
    if (rc != DTK_OK) return rc;
  }
  s->wordpiece = v != nullptr;
  s->pieces_home = v && pieces_home != 0;
  return DTK_OK;
}

extern "C" int dtk_stream_set_fold(dtk_stream *s, const dtk_fold *f) {
  if (!s) return DTK_E_ARG;
  for (dtk_batch *b : s->slots) {
    const int rc = dtk_batch_set_fold(b, f);
    if (rc != DTK_OK) return rc;
  }
  return DTK_OK;
}

extern "C" int dtk_stream_pieces(dtk_stream *s, dtk_piece_view *o) {
  if (!s || !o) return DTK_E_ARG;
  if (!s->cur.pieces_set) return DTK_E_STATE;
  *o = s->cur.pieces;
  return DTK_OK;
}

static dtk_stream_carry carry_of(const DtkPosCarry &c) {
  return dtk_stream_carry{c.posC, c.sentB, c.init, c.pos_nonempty, c.sent_nonempty};
}

extern "C" int dtk_stream_offsets(dtk_stream *s, dtk_stream_offs *o) {
  if (!s || !o) return DTK_E_ARG;
  if (!s->cur.offs_set) return DTK_E_STATE;
  const SoView &v = s->cur.offs;
  static_assert(sizeof(dtk_off_block64) == sizeof(DtkOffBlock64) && sizeof(dtk_off_block64) == 24, "the kernels' block head is the header's");
  o->n_tok = v.t->n_tok; o->n_sent = v.t->n_sent; o->n_text = v.t->n_text;
  o->tok_rstart = v.rstart; o->tok_rend = v.rend;
  o->tok_rblk = v.words; o->tok_rblk_head = reinterpret_cast<const dtk_off_block64 *>(v.heads);
  o->sent = v.sent; o->text_tok_end = v.ttok; o->text_sent_end = v.tsent;
  o->carry_in = carry_of(v.t->carry_in); o->carry_out = carry_of(v.t->carry_out);
  return DTK_OK;
}

static dtk_stream_sen_carry sen_carry_of(const DtkSenCarry &c) {
  return dtk_stream_sen_carry{c.open, 0u, c.bstart, c.bend, c.rstart, c.rend};
}

extern "C" int dtk_stream_sentences(dtk_stream *s, dtk_stream_sens *o) {
  if (!s || !o) return DTK_E_ARG;
  if (!s->cur.sens_set) return DTK_E_STATE;
  const SsView &v = s->cur.sens;
  static_assert(sizeof(dtk_stream_sen_carry) == sizeof(DtkSenCarry) && sizeof(dtk_stream_sen_carry) == 40, "the kernels' carry is the header's");
  o->n_sen = v.t->n_sen; o->n_text = v.t->n_text;
  o->sen_tok_end = v.tok_end;
  o->sen_bstart = v.bstart; o->sen_bend = v.bend; o->sen_rstart = v.rstart; o->sen_rend = v.rend;
  o->text_sen_end = v.tse;
  o->carry_in = sen_carry_of(v.t->carry_in); o->carry_out = sen_carry_of(v.t->carry_out);
  return DTK_OK;
}

extern "C" int dtk_stream_positions(dtk_stream *s, dtk_stream_pos *o) {
  if (!s || !o) return DTK_E_ARG;
  if (!s->cur.pos) return DTK_E_STATE;
  const DtkPosTrailer &t = *s->cur.pos;
  o->splice_pos = t.splice_pos; o->splice_sent = t.splice_sent;
  o->open_pos = s->cur.out + t.out_len; o->open_pos_len = t.open_pos_len;
  o->open_sent = o->open_pos + t.open_pos_len; o->open_sent_len = t.open_sent_len;
  o->carry_in = carry_of(t.carry_in); o->carry_out = carry_of(t.carry_out);
  return DTK_OK;
}

// The one place that splices: out with the held prefixes at the two offsets (the position line comes first), then
// the open fragments join what is held.
extern "C" int dtk_stream_emit(dtk_stream *s, dtk_write_fn w, void *user) {
  if (!s || !w) return DTK_E_ARG;
  if (!s->cur.pos || s->cur.emitted) return DTK_E_STATE;
  const DtkPosTrailer &t = *s->cur.pos;
  s->cur.emitted = true;
  uint64_t at = 0;
  int rc;
  std::string *held[2] = {&s->held_pos, &s->held_sent};
  const uint64_t splice[2] = {t.splice_pos, t.splice_sent};
  for (int i = 0; i < 2; i++) {
    if (splice[i] == UINT64_MAX) continue;
    if (splice[i] < at || splice[i] > t.out_len) return DTK_E_STATE;
    if (splice[i] > at && (rc = w(user, s->cur.out + at, (size_t)(splice[i] - at))) != DTK_OK) return rc;
    at = splice[i];
    if (!held[i]->empty() && (rc = w(user, reinterpret_cast<const uint8_t *>(held[i]->data()), held[i]->size())) != DTK_OK) return rc;
    held[i]->clear();
  }
  if (t.out_len > at && (rc = w(user, s->cur.out + at, (size_t)(t.out_len - at))) != DTK_OK) return rc;
  const char *open = reinterpret_cast<const char *>(s->cur.out + t.out_len);
  s->held_pos.append(open, (size_t)t.open_pos_len);
  s->held_sent.append(open + t.open_pos_len, (size_t)t.open_sent_len);
  return DTK_OK;
}

namespace {
// DTK_ST_EMPTY_TEXT for the calls of a slice up to the cursor `upto`, in the stream's terms: SentenceEnd / TextEnd while
// the current text has no token (token_writer.go:108,135,145); has_tok: what the stream carried in.
bool empty_text_upto(const dtk_result_view &v, uint32_t upto, bool last, bool has_tok) {
  const uint64_t nt = v.tok_off[1];
  const bool blocked = !v.tok_bend && v.tok_bblk;
  auto tok_end = [&](uint64_t i) { return blocked ? (uint32_t)dtk_blk_end(v.tok_bblk, v.tok_bblk_head, i) : v.tok_bend[i]; };
  uint64_t k = 0;
  uint32_t j = v.evl_off[0];
  const uint32_t j1 = v.evl_off[1];
  bool bad = false;
  while (k < nt || j < j1) {
    const uint32_t none = 0xFFFFFFFFu;
    const uint32_t pt = k < nt ? tok_end(k) : none, pe = j < j1 ? v.evl_pos[j] : none;
    const uint32_t p = pt < pe ? pt : pe;
    if (p > upto) break;
    const uint32_t e = pe == p ? v.evl_kind[j++] : 0u;
    if ((e & DTK_EVL_SEOT) && !has_tok) bad = true;
    if (e & DTK_EVL_TEOT) { if (!has_tok) bad = true; has_tok = false; }
    if (pt == p) { has_tok = true; k++; }
    if ((e & DTK_EVL_SEPS) && !has_tok) bad = true;
  }
  if (last && upto == 0xFFFFFFFFu && (v.doc_tail[0] & 3u) && !has_tok) bad = true;
  return bad;
}

struct Run {
  dtk_stream *s = nullptr;
  dtk_read_fn read_fn = nullptr; void *read_user = nullptr;
  dtk_stream_slice_fn slice_fn = nullptr; void *slice_user = nullptr;
  bool eof = false;
  std::vector<uint32_t> len;     // bytes in each slot's buffer
  std::vector<uint8_t> touched;  // the slot's batch may have work in flight
  // the stream's state between slices
  bool have_carry = false;
  DtkLaneState carry{};
  bool has_tok = false;          // the current text has had a token
  uint32_t status = 0;
  // position rendering: the bound of an integer's size.  posC counts runes of windows that begin at or behind the
  // `first` of the last slice in which a TextEnd fired; `te_from` is that of the last such slice the host has seen
  // delivered (0: none yet), so posC of a slice being enqueued stays below its cut - te_from, plus what the run began with.
  bool is_matrix = false;
  bool nl = false;               // the run's NEWLINE_AFTER_EOT (offset delivery)
  uint64_t te_from = 0, posc0 = 0;

  uint8_t *bytes(uint32_t slot) { return s->buf[slot]->as<uint8_t>(); }
  bool pos_render() const { return s->bytes == SliceRequest::kPosBytes; }
  bool writer_chain() const { return pos_render() || s->offs || s->sens; }  // the writer's state is chained on the device

  // window k into its slot: the tail of window k - 1 (null: the stream's beginning), then fresh bytes.  Returns the
  // fresh bytes read.
  uint64_t fill(uint32_t slot, const uint8_t *prev_tail) {
    const uint64_t W = s->S + kTail;
    uint64_t at = 0;
    if (prev_tail) { memcpy(bytes(slot), prev_tail, kTail); at = kTail; }
    const uint64_t at0 = at;
    while (!eof && at < W) {
      const size_t n = read_fn(read_user, bytes(slot) + at, (size_t)(W - at));
      if (n == 0 || n > W - at) { eof = true; break; }
      at += n;
    }
    len[slot] = (uint32_t)at;
    return at - at0;
  }
  int upload(uint32_t slot) {
    const uint64_t off[2] = {0, len[slot]};
    touched[slot] = 1;
    return dtk_batch_set_input(s->slots[slot], bytes(slot), off, 1);
  }

  // a slice that has been enqueued
  struct Slice {
    uint32_t slot = 0, first = 0;
    uint64_t base = 0, k = 0;
    bool open = false, ended = false, carried = false;
    DtkStreamCut c{};
  };
  // Finishes the slice (finish(): repairs, the EOT kernel, larger arrays), takes its cut block -- what the next slice
  // starts from -- and starts its results on their way home.
  int take_cut(Slice &x) {
    dtk_batch *b = s->slots[x.slot];
    int rc = batch_cut(b, &x.c);
    if (rc != DTK_OK) return rc;
    if ((x.open || x.carried) && !x.c.valid) return DTK_E_STATE;
    // (no cut although bytes follow: the walk closed the document in front of S -- a window overflow, a walk that left
    //  the table -- as the reference ends there)
    x.ended = !x.open || x.c.cut == 0xFFFFFFFFu;
    if (!x.ended) {
      carry = DtkLaneState{x.c.p, x.c.t, x.c.aux, x.c.flags};
      have_carry = true;
    }
    const uint32_t cut = x.ended ? len[x.slot] : x.c.cut;
    SliceRequest q;
    q.first = x.first; q.cut = cut; q.last = x.ended;
    q.bytes = s->bytes; q.bits = s->bits;
    q.offs = s->offs; q.form = s->offs_form;
    q.is_matrix = is_matrix; q.nl = nl;
    if (pos_render()) {
      q.digits = 2;  // ("-1")
      for (uint64_t v = x.base + cut - te_from + posc0; v >= 10u; v /= 10u) q.digits++;
    }
    q.sens = s->sens; q.base = x.base;
    if (writer_chain()) {
      const uint64_t slots = (uint64_t)s->depth + 1u, slot = x.k % slots;
      q.carry_in = s->d_carry + slot; q.carry_out = s->d_carry + (slot + 1u) % slots;
      if (s->sens) { q.sen_carry_in = s->d_sen_carry + slot; q.sen_carry_out = s->d_sen_carry + (slot + 1u) % slots; }
    }
    batch_set_slice_request(b, q);
    return dtk_batch_download_begin(b);
  }
  // hands the slice over (its successor may be walking meanwhile)
  int deliver(const Slice &x) {
    dtk_batch *b = s->slots[x.slot];
    dtk_stream_slice sl{};
    sl.base = x.base; sl.first = x.first; sl.len = len[x.slot]; sl.text = bytes(x.slot);
    sl.last = x.ended ? 1u : 0u;
    sl.cut = x.ended ? sl.len : x.c.cut;
    int rc = dtk_batch_result_host(b, &sl.view);
    if (rc != DTK_OK) return rc;
    if (sl.view.n_exact) return DTK_E_IRREGULAR;
    uint32_t st = sl.view.status[0];
    if (x.carried) {
      // the lane that walked from the carried record took the writer for new: its bit is decided here
      st |= x.c.walker_status & ~(uint32_t)DTK_ST_EMPTY_TEXT;
      if ((x.c.walker_status & DTK_ST_EMPTY_TEXT) && empty_text_upto(sl.view, x.c.walker_end, x.ended, has_tok))
        st |= DTK_ST_EMPTY_TEXT;
    }
    sl.status = st;
    status |= st;
    // "the current text has had a token" behind this slice
    const uint64_t nt = sl.view.tok_off[1], nx = sl.view.text_off[1];
    const uint64_t n_teot = nx - ((x.ended && (sl.view.doc_tail[0] & DTK_TAIL_E)) ? 1u : 0u);
    has_tok = n_teot ? nt > sl.view.text_tok_end[n_teot - 1] : (has_tok || nt > 0);
    if (n_teot || nx) te_from = x.base + x.first;
    if (s->bytes == SliceRequest::kPlainBytes && (rc = batch_render_out(b, &sl.out, &sl.out_len)) != DTK_OK) return rc;
    if (pos_render()) {
      if ((rc = batch_pos_out(b, &s->cur.out, &s->cur.pos)) != DTK_OK) return rc;  // (cur is as it was: empty)
      sl.out = s->cur.out; sl.out_len = s->cur.pos->out_len;
    }
    if (s->offs) {
      if ((rc = batch_offs_out(b, &s->cur.offs)) != DTK_OK) return rc;
      s->cur.offs_set = true;
    }
    if (s->sens) {
      if ((rc = batch_sens_out(b, &s->cur.sens)) != DTK_OK) return rc;
      s->cur.sens_set = true;
    }
    if (s->vocab) {
      // (the lookup was enqueued with the slice's download, take_cut; this waits for it, so a tally holds the slice)
      rc = s->ids_home ? dtk_batch_token_ids_host(b, &s->cur.ids) : dtk_batch_token_ids_device(b, &s->cur.ids);
      if (rc != DTK_OK) return rc;
      if (!s->ids_home) s->cur.ids.tok_id = nullptr;  // (host pointers only)
      s->cur.ids_set = true;
    }
    if (s->wordpiece) {
      rc = s->pieces_home ? dtk_batch_pieces_host(b, &s->cur.pieces) : dtk_batch_pieces_device(b, &s->cur.pieces);
      if (rc != DTK_OK) return rc;
      if (!s->pieces_home) s->cur.pieces.piece_off = nullptr, s->cur.pieces.piece_id = nullptr, s->cur.pieces.piece_bend = nullptr;
      s->cur.pieces_set = true;
    }
    rc = slice_fn ? slice_fn(slice_user, &sl) : DTK_OK;
    s->cur = {};
    return rc;
  }
};
}  // namespace

extern "C" int dtk_stream_run(dtk_stream *s, const dtk_model *m, dtk_read_fn read_fn, void *read_user, uint32_t flags,
                              dtk_stream_slice_fn slice_fn, void *slice_user, uint32_t *status) {
  if (!s || !m || !read_fn || (flags & ~(uint32_t)31u)) return DTK_E_ARG;
  if (s->bytes == SliceRequest::kPosBytes && ((flags ^ s->bits) & DTK_NEWLINE_AFTER_EOT)) return DTK_E_ARG;  // the rule is part of the rendering
  if (status) *status = 0;
  const uint32_t depth = s->depth;
  Run r;
  r.s = s; r.read_fn = read_fn; r.read_user = read_user; r.slice_fn = slice_fn; r.slice_user = slice_user;
  r.len.assign(depth, 0);
  r.touched.assign(depth, 0);
  s->held_pos.clear(); s->held_sent.clear();
  s->cur = {};
  r.is_matrix = std::strcmp(dtk_model_type(m), "MATOK") == 0;
  r.nl = (flags & DTK_NEWLINE_AFTER_EOT) != 0;
  if (r.writer_chain()) {
    // a new writer: {posC 0, sentB, init} (token_writer.go:38-42) in slot 0 of the chain
    const DtkPosCarry c0{g_dbg.sp_posc0, 1u, 1u, 0u, 0u};
    if (r.pos_render()) r.posc0 = (uint64_t)(c0.posC < 0 ? -c0.posC : c0.posC);
    HIP_TRY(hipMemcpy(s->d_carry.p, &c0, sizeof(c0), hipMemcpyHostToDevice));
    const DtkSenCarry s0{};  // no row is open
    if (s->sens) HIP_TRY(hipMemcpy(s->d_sen_carry.p, &s0, sizeof(s0), hipMemcpyHostToDevice));
  }
  // (the writer's rune offsets are the host's: the compaction writes the byte offsets only)
  const uint32_t run_flags = DTK_NO_RUNE_OFFSETS;
  r.fill(0, nullptr);
  int rc = r.upload(0);
  Run::Slice prev;
  for (uint64_t k = 0; rc == DTK_OK; k++) {
    const uint32_t slot = (uint32_t)(k % depth), next = (uint32_t)((k + 1) % depth);
    // with two buffers window k + 1 goes where slice k - 1 lies: that one is handed over first
    if (k > 0 && depth == 2 && ((rc = r.take_cut(prev)) != DTK_OK || (rc = r.deliver(prev)) != DTK_OK || prev.ended)) break;
    // The predecessor's cut: slice k starts from it.  It is taken behind the read of window k + 1, which then runs
    // beside the predecessor's walk -- except with position rendering, whose download (the capacity bound of the
    // position lines: some 4 bytes per input byte) is a slice's longest leg: there the cut comes first, and the read
    // runs beside that download (profiles/stream_positions.txt).
    const bool cut_first = r.pos_render();
    auto cut_prev = [&]() -> bool {  // false: the loop ends here
      if ((rc = r.take_cut(prev)) != DTK_OK) return false;
      if (prev.ended) { rc = r.deliver(prev); return false; }
      return true;
    };
    if (k > 0 && depth > 2 && cut_first && !cut_prev()) break;
    bool open = false;
    if (r.len[slot] == s->S + kTail && !r.eof) {
      open = r.fill(next, r.bytes(slot) + s->S) > 0;
      if (open && (rc = r.upload(next)) != DTK_OK) break;
    }
    if (k > 0 && depth > 2 && !cut_first && !cut_prev()) break;
    Run::Slice cur;
    cur.slot = slot; cur.base = k * s->S; cur.k = k; cur.open = open;
    cur.carried = r.have_carry; cur.first = r.have_carry ? r.carry.p : 0u;
    if ((rc = batch_set_slice(s->slots[slot], open ? (uint32_t)s->S : 0u, r.have_carry ? &r.carry : nullptr)) != DTK_OK ||
        (rc = dtk_batch_run(m, s->slots[slot], run_flags)) != DTK_OK)
      break;
    if (k > 0 && depth > 2 && (rc = r.deliver(prev)) != DTK_OK) break;  // (under the walk of slice k)
    if (!open) {  // the stream's last slice
      if ((rc = r.take_cut(cur)) == DTK_OK) rc = r.deliver(cur);
      break;
    }
    prev = cur;
  }
  // nothing of this run stays in flight (an error, or a slice that ended the stream early with its successor uploaded)
  for (uint32_t q = 0; q < depth; q++)
    if (r.touched[q]) {
      (void)dtk_batch_sync(s->slots[q]);
      (void)batch_set_slice(s->slots[q], 0u, nullptr);
      batch_set_slice_request(s->slots[q], SliceRequest{});
    }
  if (status) *status = r.status;
  return rc;
}
