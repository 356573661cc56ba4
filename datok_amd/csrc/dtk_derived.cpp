// dtk_derived.cpp -- the tables a finished run's download derives from its result arrays, on the download stream behind
// finish(): the sentence table, the tokens' ids, their WordPiece pieces and the model input rows.  Each is a DerivedBlock
// (dtk_mirror.h; the protocol: DESIGN.md section 2.13) with an *_enqueue, which never waits, and a *_finish, which does.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dtk_host.h"

namespace {
// `enqueue`, then the wait for it: the step of derived_complete
template <class Enqueue>
auto and_wait(DerivedBlock &L, Enqueue enqueue) {
  return [&L, enqueue] { const int rc = enqueue(); return rc != DTK_OK ? rc : L.wait(); };
}

// ---- DTK_R_SENTENCES: the sentence table (dtk_sentences.hip; the definition is in include/datok_gpu.h)

// The table's block and its page-locked copy, for `rows` rows and `texts` text rows: both with room for it.
int sen_describe(dtk_batch *b, uint64_t rows, uint64_t texts) {
  dtk_batch::Sen &L = b->sen;
  L.clear();
  L.add(L.off, (uint64_t)b->n_docs + 1);
  L.add(L.tok_end, rows); L.add(L.bstart, rows); L.add(L.bend, rows); L.add(L.rstart, rows); L.add(L.rend, rows);
  L.add(L.tse, texts); L.add(L.cnt, 1);
  return L.fit();
}

void sen_view(const dtk_batch *b, void *block, dtk_sentence_view *o) {  // block: sen.d or sen.h
  const dtk_batch::Sen &L = b->sen;
  const bool runes = !(b->last_flags & DTK_NO_RUNE_OFFSETS);
  o->n_sen = L.n;
  o->sen_off = L.in(block, L.off);
  o->sen_tok_end = L.in(block, L.tok_end); o->sen_bstart = L.in(block, L.bstart); o->sen_bend = L.in(block, L.bend);
  o->sen_rstart = runes ? L.in(block, L.rstart) : nullptr; o->sen_rend = runes ? L.in(block, L.rend) : nullptr;
  o->text_sen_end = L.in(block, L.tse);
}

// The rows of documents the exact pass walked come from their calls: the table is taken apart on the host, their
// rows are put in place of what their bitmaps gave, and the whole goes back to the device.  Exact, and slow.
int sen_splice_exact(dtk_batch *b) {
  const uint32_t nd = b->n_docs, ne = (uint32_t)b->h_exact_ids.size();
  const bool runes = !(b->last_flags & DTK_NO_RUNE_OFFSETS);
  std::vector<uint64_t> csr(3 * ((size_t)nd + 1));
  HIP_TRY(hipMemcpy(csr.data(), b->d_csr, csr.size() * 8, hipMemcpyDeviceToHost));
  const uint64_t *tok_off = csr.data(), *text_off = csr.data() + 2 * ((size_t)nd + 1);
  dtk_batch::Sen &L = b->sen;  // (as the kernels filled it; described anew below, for the spliced rows)
  const uint64_t *o_off = L.host(L.off);
  struct Row { uint32_t tok_end, bstart, bend; int32_t rstart, rend; };
  std::vector<Row> rows;
  std::vector<uint64_t> off((size_t)nd + 1, 0);
  std::vector<uint32_t> tse(L.host(L.tse), L.host(L.tse) + L.cap(L.tse));
  rows.reserve((size_t)L.n);
  uint32_t e = 0;
  std::vector<uint32_t> firsts, bs, be, ttok;
  std::vector<int32_t> rs, re;
  for (uint32_t d = 0; d < nd; d++) {
    off[d] = rows.size();
    if (e < ne && b->h_exact_ids[e] == d) {
      firsts.clear();
      uint32_t k = 0;
      bool open = false;
      for (uint64_t c = b->h_exact_off[e]; c < b->h_exact_off[e + 1]; c++) {
        if (b->h_calls[c].kind == 0) { if (!open) firsts.push_back(k); open = true; k++; }
        else open = false;
      }
      e++;
      const uint64_t t0 = tok_off[d], nt = tok_off[d + 1] - t0;
      if (k != nt) return DTK_E_STATE;  // (the exact pass wrote one token row per Token call)
      bs.resize(nt); be.resize(nt); rs.assign(nt, 0); re.assign(nt, 0);
      if (nt) {
        HIP_TRY(hipMemcpy(bs.data(), b->d_bstart + t0, nt * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(be.data(), b->d_bend + t0, nt * 4, hipMemcpyDeviceToHost));
        if (runes) {
          HIP_TRY(hipMemcpy(rs.data(), b->d_rstart + t0, nt * 4, hipMemcpyDeviceToHost));
          HIP_TRY(hipMemcpy(re.data(), b->d_rend + t0, nt * 4, hipMemcpyDeviceToHost));
        }
      }
      for (size_t i = 0; i < firsts.size(); i++) {
        const uint32_t f = firsts[i], end = i + 1 < firsts.size() ? firsts[i + 1] : (uint32_t)nt;
        rows.push_back(Row{end, bs[f], be[end - 1], rs[f], re[end - 1]});
      }
      const uint64_t x0 = text_off[d], nx = text_off[d + 1] - x0;
      ttok.resize(nx);
      if (nx) HIP_TRY(hipMemcpy(ttok.data(), b->d_ttok + x0, nx * 4, hipMemcpyDeviceToHost));
      for (uint64_t g = 0; g < nx && x0 + g < tse.size(); g++)
        tse[x0 + g] = (uint32_t)(std::lower_bound(firsts.begin(), firsts.end(), ttok[g]) - firsts.begin());
    } else {
      for (uint64_t i = o_off[d]; i < o_off[d + 1]; i++)
        rows.push_back(Row{L.host(L.tok_end)[i], L.host(L.bstart)[i], L.host(L.bend)[i], L.host(L.rstart)[i], L.host(L.rend)[i]});
    }
  }
  off[nd] = rows.size();
  const uint64_t n = rows.size();
  const int rc = sen_describe(b, std::max<uint64_t>(n, 1), tse.size());
  if (rc != DTK_OK) return rc;
  memset(L.h.p, 0, (size_t)L.bytes);
  std::copy(off.begin(), off.end(), L.host(L.off));
  for (uint64_t i = 0; i < n; i++) {
    L.host(L.tok_end)[i] = rows[i].tok_end; L.host(L.bstart)[i] = rows[i].bstart; L.host(L.bend)[i] = rows[i].bend;
    L.host(L.rstart)[i] = rows[i].rstart; L.host(L.rend)[i] = rows[i].rend;
  }
  std::copy(tse.begin(), tse.end(), L.host(L.tse));
  *L.host(L.cnt) = (uint32_t)n;
  HIP_TRY(hipMemcpy(L.d.p, L.h.p, (size_t)L.bytes, hipMemcpyHostToDevice));
  L.all_home();
  L.n = n;
  L.gen++;  // (a rewrite: what read the table as the kernels left it is stale)
  return DTK_OK;
}

// The table, complete: on the device, and (home) in the page-locked block.
int sen_finish(dtk_batch *b, bool home) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if (!b->h_exact_ids.empty()) home = true;  // (the splice works on the host copy)
  dtk_batch::Sen &L = b->sen;
  // more rows than the bound (not expected of regular documents): the kernels wrote nothing; again, for n rows
  rc = derived_complete(L, and_wait(L, [&] { return sen_enqueue(b, home); }),
                        [&](uint64_t &n) { return L.done || (n = *L.host(L.cnt)) <= L.cap(L.tok_end); });
  if (rc != DTK_OK || L.done) return rc;  // (done: the count was looked at before, this call only brought the block home)
  L.n = *L.host(L.cnt);
  if (!b->h_exact_ids.empty() && (rc = sen_splice_exact(b)) != DTK_OK) return rc;
  L.done = true;
  return DTK_OK;
}

// ---- dtk_batch_set_vocab: the tokens' ids (dtk_tokenid.hip; the definition is in include/datok_gpu.h)

// Enqueues on the download stream what is still missing of: the lookup (once per run: it also feeds the tally), the
// copy of the unknown counter, and (home) the copy of the ids.  The run is complete (finish()), so the token count is
// final and the block is sized exactly.
int ids_enqueue(dtk_batch *b, bool home) {
  if (!b->vocab || (b->last_flags & DTK_NO_BYTE_OFFSETS)) return DTK_E_STATE;  // (the keys are cut out with tok_bstart / tok_bend)
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  dtk_batch::Ids &L = b->ids;
  const uint64_t nt = b->totals.n_tokens;
  if (!L.built) {
    L.clear();
    L.add(L.cnt, 1); L.add(L.id, nt);
    const int rc = L.fit();
    if (rc != DTK_OK) return rc;
    HIP_TRY(hipMemsetAsync(L.dev(L.cnt), 0, sizeof(uint64_t), b->dl_stream));
    DtkTokenIdArgs a{};
    a.text = b->d_text; a.total = b->total; a.doc_off = b->d_off; a.n_docs = b->n_docs;
    a.tok_off = b->d_tok_off; a.tok_bstart = b->d_bstart; a.tok_bend = b->d_bend; a.n_tok = nt;
    if (b->n_invalid) { const DtkSym s = sym_of(b); a.sym_base = s.base; a.sym_lut = s.lut; }
    a.vocab = b->vocab->dev;
    if (b->fold) a.fold = b->fold->dev;
    a.tok_id = L.dev(L.id);
    a.n_unknown = reinterpret_cast<unsigned long long *>(L.dev(L.cnt));
    a.tally = b->tally ? b->tally->d_counts.p : nullptr;
    if (dtk_launch_token_ids(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "token ids");
    L.launched();
    L.bring(L.cnt, 1);
  }
  if (home) L.bring(L.id, nt);
  return L.record(b->dl_stream);
}

// The ids, complete: on the device, and (home) in the page-locked block.
int ids_finish(dtk_batch *b, bool home, dtk_token_id_view *o) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  dtk_batch::Ids &L = b->ids;
  if ((rc = ids_enqueue(b, home || b->ids_home)) != DTK_OK || (rc = L.wait()) != DTK_OK) return rc;
  o->n_tok = b->totals.n_tokens;
  o->n_unknown = *L.host(L.cnt);
  o->tok_id = L.in(home ? L.h.p : static_cast<void *>(L.d.p), L.id);
  return DTK_OK;
}

// ---- dtk_batch_set_wordpiece: the tokens' pieces (dtk_wordpiece.hip; the definition is in include/datok_gpu.h)

// Pieces the first block of a run holds: the count is known only behind the split, and nothing here waits for it.
// Running text splits few of its tokens, so half as many pieces again as tokens; a run that needs more says so
// (pieces.need) and is split again into a block of that size -- which the batch's later runs start with, so a
// pipeline's slices of one kind of text pay for the second split once per slot.
uint64_t wp_cap_of(const dtk_batch *b) {
  const uint64_t nt = b->totals.n_tokens;
  return std::max(b->pieces.need, nt + nt / 2 + 64);
}

// Enqueues on the download stream what is still missing of: the split (once per run and block), the copy of the two
// counters, and (home) the copies of piece_off and of the pieces -- as many as there are tokens, the rest follows
// when the count is known (wp_finish).
int wp_enqueue(dtk_batch *b, bool home) {
  if (!b->wp_vocab || (b->last_flags & DTK_NO_BYTE_OFFSETS)) return DTK_E_STATE;  // (the keys are cut out with tok_bstart / tok_bend)
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  dtk_batch::Pieces &L = b->pieces;
  const uint64_t nt = b->totals.n_tokens;
  if (!L.built) {
    const uint64_t tiles = dtk_wp_tiles(nt), cap = wp_cap_of(b);
    int rc;
    L.clear();
    L.add(L.cnt, 2); L.add(L.off, nt + 1); L.add(L.id, cap); L.add(L.bend, cap);
    if ((rc = L.fit()) != DTK_OK || (rc = b->d_wp_ws.fit(tiles + 1 + nt, tiles + 1 + nt + nt / 8)) != DTK_OK) return rc;
    HIP_TRY(hipMemsetAsync(L.dev(L.cnt), 0, 2 * sizeof(uint64_t), b->dl_stream));
    DtkWordPieceArgs a{};
    a.text = b->d_text; a.total = b->total; a.doc_off = b->d_off; a.n_docs = b->n_docs;
    a.tok_off = b->d_tok_off; a.tok_bstart = b->d_bstart; a.tok_bend = b->d_bend; a.n_tok = nt;
    if (b->n_invalid) { const DtkSym s = sym_of(b); a.sym_base = s.base; a.sym_lut = s.lut; }
    a.vocab = b->wp_vocab->dev;
    a.rule = b->wp_rule;
    if (b->fold) a.fold = b->fold->dev;
    a.tile_base = b->d_wp_ws.p;
    a.first = reinterpret_cast<DtkWpFirst *>(b->d_wp_ws.p + tiles + 1);
    a.cnt = reinterpret_cast<unsigned long long *>(L.dev(L.cnt));
    a.piece_off = L.dev(L.off); a.piece_id = L.dev(L.id); a.piece_bend = L.dev(L.bend);
    a.cap = cap;
    if (dtk_launch_wordpiece(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "wordpiece");
    L.launched();
    L.bring(L.cnt, 2);
  }
  // (The first copies bring nt ids and ends whatever the count turns out to be: with fewer pieces -- tokens of an empty
  //  key -- or a run that overflowed the block and wrote none, device memory nobody wrote comes home behind them.  No
  //  view shows it: n_pieces bounds every view, and an overflowed run is split and copied again.)
  if (home) { L.bring(L.off, nt + 1); L.bring(L.id, nt); L.bring(L.bend, nt); }
  return L.record(b->dl_stream);
}

// The pieces, complete: on the device, and (home, or pieces_home) in the page-locked block.  The view's pointers are
// the caller's choice alone: device pointers for home == false, whatever has been brought home beside them.
int wp_finish(dtk_batch *b, bool home, dtk_piece_view *o) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  const bool copies = home || b->wp_home;
  dtk_batch::Pieces &L = b->pieces;
  // more pieces than the block holds: no piece was written; once more, into a block that holds them
  rc = derived_complete(L, and_wait(L, [&] { return wp_enqueue(b, copies); }),
                        [&](uint64_t &n) { return (n = L.host(L.cnt)[0]) <= L.cap(L.id); });
  if (rc != DTK_OK) return rc;
  const uint64_t np = L.host(L.cnt)[0];
  if (copies) {  // (what the first copies left out)
    L.bring(L.id, np); L.bring(L.bend, np);
    if ((rc = L.record(b->dl_stream)) != DTK_OK || (rc = L.wait()) != DTK_OK) return rc;
  }
  void *base = home ? L.h.p : static_cast<void *>(L.d.p);
  o->n_tok = b->totals.n_tokens;
  o->n_pieces = np;
  o->n_unknown = L.host(L.cnt)[1];
  o->piece_off = L.in(base, L.off);
  o->piece_id = L.in(base, L.id);
  o->piece_bend = L.in(base, L.bend);
  return DTK_OK;
}

// ---- dtk_batch_set_encode: the model input rows (dtk_encode.hip; the definition is in include/datok_gpu.h)

bool enc_state(const dtk_batch *b) { return b->enc_on && b->wp_vocab && !(b->last_flags & DTK_NO_BYTE_OFFSETS); }

// Enqueues on the download stream what is still missing of: the split and (sentence unit) the sentence table, the encode
// (once per run, per block and per state of the tables it reads), the copy of its counters, and (home) the copies of
// unit_row_off and of as many rows as there are units -- the rest follows when the count is known (enc_finish).
// Nothing here waits.  The block is sized by n_rows <= n_units + n_pieces / step, with the bounds the host has: the
// split's capacity for the pieces, the documents or the sentence table's capacity for the units.
int enc_enqueue(dtk_batch *b, bool home) {
  if (!enc_state(b)) return DTK_E_STATE;
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  const DtkEncRule &R = b->enc_rule;
  const bool sentences = R.unit == DTK_ENC_SENTENCE, words = (R.flags & DTK_ENC_WORD_IDS) != 0;
  const dtk_batch::Sen &S = b->sen;
  const dtk_batch::Pieces &P = b->pieces;
  int rc;
  if ((rc = wp_enqueue(b, b->wp_home)) != DTK_OK) return rc;
  if (sentences) {
    // documents the exact pass walked get their rows on the host (sen_splice_exact): the encode waits until somebody
    // asks for it
    if (!b->h_exact_ids.empty() && !S.done) return DTK_OK;
    if (!S.built && (rc = sen_enqueue(b, false)) != DTK_OK) return rc;
  }
  dtk_batch::Enc &L = b->enc;
  const DerivedReads now{P.gen, sentences ? S.gen : 0u};
  if (L.read.stale(now.a, now.b)) L.built = false;
  const bool launch = !L.built;
  if (launch) {
    const uint64_t units_cap = sentences ? S.cap(S.tok_end) : b->n_docs;
    uint64_t rows = units_cap + ((R.flags & DTK_ENC_FIRST_WINDOW) ? 0u : P.cap(P.id) / R.step);
    rows = (std::max<uint64_t>(std::max(rows, L.need), 1) + 3u) & ~3ull;  // (whole 16 bytes of ids: word_id stays aligned)
    const uint64_t cells = rows * R.max_len, tiles = dtk_enc_tiles(units_cap);
    const uint64_t ws = tiles + 1 + units_cap * (sizeof(DtkEncUnit) / 8);
    static_assert(sizeof(DtkEncUnit) % 8 == 0, "the workspace is laid out in 64-bit words");
    L.clear();
    L.add(L.ids, cells); L.add(L.word, words ? cells : 0); L.add(L.piece0, rows); L.add(L.off, units_cap + 1); L.add(L.len, rows);
    if ((rc = L.fit(false)) != DTK_OK || (rc = b->d_enc_ws.fit(ws, ws + ws / 8)) != DTK_OK ||
        (rc = b->d_enc_cnt.fit(4, 4)) != DTK_OK || (rc = b->h_enc_cnt.fit(4 * sizeof(uint64_t))) != DTK_OK)
      return rc;
    HIP_TRY(hipMemsetAsync(b->d_enc_cnt.p, 0, 4 * sizeof(uint64_t), b->dl_stream));
    DtkEncodeArgs a{};
    a.rule = R;
    a.tok_off = b->d_tok_off; a.n_docs = b->n_docs; a.n_tok = b->totals.n_tokens;
    if (sentences) {
      a.sen_off = S.dev(S.off); a.sen_tok_end = S.dev(S.tok_end); a.sen_count = S.dev(S.cnt);
      a.sen_cap = units_cap;
    }
    a.piece_off = P.dev(P.off); a.piece_id = P.dev(P.id); a.piece_cap = P.cap(P.id);
    a.units_cap = units_cap; a.rows_cap = rows;
    a.tile_base = b->d_enc_ws.p;
    a.unit = reinterpret_cast<DtkEncUnit *>(b->d_enc_ws.p + tiles + 1);
    a.cnt = reinterpret_cast<unsigned long long *>(b->d_enc_cnt.p);
    a.unit_row_off = L.dev(L.off); a.input_ids = L.dev(L.ids); a.row_len = L.dev(L.len); a.row_piece0 = L.dev(L.piece0);
    a.word_id = words ? L.dev(L.word) : nullptr;
    if (dtk_launch_encode(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "encode");
    L.launched();
    L.read = now;
    HIP_TRY(hipMemcpyAsync(b->h_enc_cnt.p, b->d_enc_cnt.p, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, b->dl_stream));
  }
  if (home) {
    // (as with the pieces: rows nobody wrote may come home behind the written ones, and no view shows them)
    if ((rc = L.h.fit((size_t)L.bytes)) != DTK_OK) return rc;
    const uint64_t first = std::min(L.cap(L.off) - 1, L.cap(L.len));
    L.bring(L.ids, first * R.max_len); L.bring(L.word, first * R.max_len); L.bring(L.piece0, first);
    L.bring(L.off, L.cap(L.off)); L.bring(L.len, first);
  }
  return L.record(b->dl_stream, launch);
}

// The rows, complete: on the device, and (home, or rows_home) in the page-locked block.  The pieces and the sentence
// table are completed first; an encode that read an earlier state of either, or outgrew its block, is done again.
int enc_finish(dtk_batch *b, bool home, dtk_encode_view *o) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if (!enc_state(b)) return DTK_E_STATE;
  dtk_batch::Enc &L = b->enc;
  if ((rc = L.wait()) != DTK_OK) return rc;  // (nothing reads the tables while they are made anew)
  dtk_piece_view pieces;
  if ((rc = wp_finish(b, false, &pieces)) != DTK_OK) return rc;
  const DtkEncRule &R = b->enc_rule;
  if (R.unit == DTK_ENC_SENTENCE && (rc = sen_finish(b, false)) != DTK_OK) return rc;
  const bool copies = home || b->enc_home;
  const uint64_t *cnt = nullptr;
  // the verdict `ok` is missing: no row was written; once more, into a block that holds them
  rc = derived_complete(L, and_wait(L, [&] { return enc_enqueue(b, copies); }),
                        [&](uint64_t &n) { cnt = b->h_enc_cnt.as<uint64_t>(); n = cnt[0]; return cnt[3] != 0; });
  if (rc != DTK_OK) return rc;
  const uint64_t n_rows = cnt[0], n_units = cnt[2];
  if (copies) {  // (what the first copies left out)
    L.bring(L.ids, n_rows * R.max_len); L.bring(L.word, n_rows * R.max_len); L.bring(L.piece0, n_rows);
    L.bring(L.off, n_units + 1); L.bring(L.len, n_rows);
    if ((rc = L.record(b->dl_stream)) != DTK_OK || (rc = L.wait()) != DTK_OK) return rc;
  }
  void *base = home ? L.h.p : static_cast<void *>(L.d.p);
  o->n_units = n_units; o->n_rows = n_rows; o->n_cut = cnt[1];
  o->max_len = R.max_len;
  o->unit_row_off = L.in(base, L.off);
  o->input_ids = L.in(base, L.ids);
  o->row_len = L.in(base, L.len);
  o->row_piece0 = L.in(base, L.piece0);
  o->word_id = (R.flags & DTK_ENC_WORD_IDS) ? L.in(base, L.word) : nullptr;
  return DTK_OK;
}
}  // namespace

// Enqueues on the download stream what is still missing of: the table's kernels (once per run and block), and the copy
// of the whole block (home) or of its count word.  The run is complete (finish()).
int sen_enqueue(dtk_batch *b, bool home) {
  if (b->last_flags & DTK_NO_BYTE_OFFSETS) return DTK_E_STATE;  // the table is keyed on tok_bend
  const uint64_t n_bits = b->total + b->n_docs;
  // every row is an int the writer's Token closure pushes to sent[]: n_sent bounds the rows of regular documents, and
  // the count word backs the bound up (sen_finish)
  uint64_t rows = g_dbg.sen_cap >= 0 ? (uint64_t)g_dbg.sen_cap : b->totals.n_sent;
  dtk_batch::Sen &L = b->sen;
  rows = std::max<uint64_t>(std::max(rows, L.need), 1);
  if (n_bits > 0xFFFFFFFFull || rows > 0xFFFFFFFFull) return DTK_E_CAPACITY;
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  if (!L.built || (!L.done && rows > L.cap(L.tok_end))) {
    const uint32_t tiles = dtk_sentences_tiles(n_bits, b->bit_words);
    const uint64_t ws = 3 * rows + 2 * (uint64_t)tiles;
    int rc;
    if ((rc = sen_describe(b, rows, b->totals.n_texts)) || (rc = b->d_sen_ws.fit(ws, ws + ws / 8))) return rc;
    DtkSentencesArgs a{};
    a.bits = b->d_bits; a.bit_words = b->bit_words; a.n_docs = b->n_docs; a.doc_off = b->d_off; a.n_bits = n_bits;
    a.n_tiles = tiles; a.cap = (uint32_t)rows;
    a.tok_off = b->d_tok_off; a.text_off = b->d_text_off; a.tok_bstart = b->d_bstart; a.tok_bend = b->d_bend;
    if (!(b->last_flags & DTK_NO_RUNE_OFFSETS)) { a.tok_rstart = b->d_rstart; a.tok_rend = b->d_rend; }
    a.text_tok_end = b->d_ttok;
    a.text_cap = L.cap(L.tse);
    a.sen_bit = b->d_sen_ws; a.sen_doc = a.sen_bit + rows; a.sen_first = a.sen_doc + rows;
    a.tile_base = a.sen_first + rows; a.tile_in = a.tile_base + tiles;
    a.count = L.dev(L.cnt); a.sen_off = L.dev(L.off);
    a.sen_tok_end = L.dev(L.tok_end); a.sen_bstart = L.dev(L.bstart); a.sen_bend = L.dev(L.bend);
    a.sen_rstart = L.dev(L.rstart); a.sen_rend = L.dev(L.rend); a.text_sen_end = L.dev(L.tse);
    if (dtk_launch_sentences(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "sentence table");
    L.launched();
    L.done = false;
  }
  if (home) {  // (the pieces in the block's order, each whole, the count word last: one range, one copy)
    L.bring(L.off, L.cap(L.off));
    L.bring(L.tok_end, L.cap(L.tok_end)); L.bring(L.bstart, L.cap(L.bstart)); L.bring(L.bend, L.cap(L.bend));
    L.bring(L.rstart, L.cap(L.rstart)); L.bring(L.rend, L.cap(L.rend));
    L.bring(L.tse, L.cap(L.tse));
  }
  L.bring(L.cnt, 1);
  return L.record(b->dl_stream);
}

int derived_enqueue(dtk_batch *b) {
  const bool keys = !(b->last_flags & DTK_NO_BYTE_OFFSETS);
  int rc;
  // the tokens' ids (dtk_batch_set_vocab): no result field, they ride in front of the fields' copies
  if (b->vocab && keys && (rc = ids_enqueue(b, b->ids_home)) != DTK_OK) return rc;
  // ... and their pieces (dtk_batch_set_wordpiece), the same way
  if (b->wp_vocab && keys && (rc = wp_enqueue(b, b->wp_home)) != DTK_OK) return rc;
  // ... and the model input rows made of them (dtk_batch_set_encode)
  return enc_state(b) ? enc_enqueue(b, b->enc_home) : DTK_OK;
}

int derived_wait(dtk_batch *b) {
  int rc = DTK_OK;
  DerivedBlock *const stages[] = {&b->sen, &b->ids, &b->pieces, &b->enc};
  for (DerivedBlock *t : stages) {
    const int r = t->wait();
    if (rc == DTK_OK) rc = r;
  }
  return rc;
}

extern "C" int dtk_batch_sentences_device(dtk_batch *b, dtk_sentence_view *o) {
  if (!b || !o) return DTK_E_ARG;
  const int rc = sen_finish(b, false);
  if (rc != DTK_OK) return rc;
  sen_view(b, b->sen.d.p, o);
  return DTK_OK;
}

extern "C" int dtk_batch_sentences_host(dtk_batch *b, dtk_sentence_view *o) {
  if (!b || !o) return DTK_E_ARG;
  const int rc = sen_finish(b, true);
  if (rc != DTK_OK) return rc;
  sen_view(b, b->sen.h.p, o);
  return DTK_OK;
}

extern "C" int dtk_batch_set_vocab(dtk_batch *b, const dtk_vocab *v, dtk_tally *t, int ids_home) {
  if (!b || (!v && t)) return DTK_E_ARG;
  if (v && (v->device != b->device || (t && (t->device != b->device || t->n_words != v->n_words)))) return DTK_E_ARG;
  const int rc = b->ids.wait();  // (a lookup under way reads the vocabulary that was attached)
  if (rc != DTK_OK) return rc;
  // (another vocabulary: the finished run, if any, is looked up anew when its ids are asked for; the same one again
  //  keeps what was computed, so a run's tokens reach a tally once)
  if (v != b->vocab) b->ids.built = false;
  b->vocab = v; b->tally = t; b->ids_home = v && ids_home != 0;
  return DTK_OK;
}

extern "C" int dtk_batch_token_ids_device(dtk_batch *b, dtk_token_id_view *o) {
  return !b || !o ? DTK_E_ARG : ids_finish(b, false, o);
}

extern "C" int dtk_batch_token_ids_host(dtk_batch *b, dtk_token_id_view *o) {
  return !b || !o ? DTK_E_ARG : ids_finish(b, true, o);
}

extern "C" int dtk_batch_set_wordpiece(dtk_batch *b, const dtk_vocab *v, const uint8_t *prefix, uint32_t prefix_len,
                                       int32_t unk_id, uint32_t max_runes, int pieces_home) {
  if (!b || (v && v->device != b->device)) return DTK_E_ARG;
  DtkWpRule rule{};
  int rc = v ? wordpiece_rule(v->n_words, prefix, prefix_len, unk_id, max_runes, &rule) : DTK_OK;
  if (rc != DTK_OK || (rc = b->pieces.wait()) != DTK_OK) return rc;  // (a split under way reads the vocabulary that was attached)
  // (the finished run, if any, is split anew under the new rule when its pieces are asked for)
  b->pieces.built = false;
  b->wp_vocab = v; b->wp_rule = rule; b->wp_home = v && pieces_home != 0;
  return DTK_OK;
}

extern "C" int dtk_batch_set_fold(dtk_batch *b, const dtk_fold *f) {
  if (!b || (f && f->device != b->device)) return DTK_E_ARG;
  int rc;
  // (a lookup or a split under way reads the fold that was attached)
  if ((rc = b->ids.wait()) != DTK_OK || (rc = b->pieces.wait()) != DTK_OK) return rc;
  // (the finished run, if any, is looked up and split anew under the new fold when its ids or pieces are asked for; the
  //  rows follow their pieces)
  if (f != b->fold) b->ids.built = b->pieces.built = false;
  b->fold = f;
  return DTK_OK;
}

extern "C" int dtk_batch_pieces_device(dtk_batch *b, dtk_piece_view *o) {
  return !b || !o ? DTK_E_ARG : wp_finish(b, false, o);
}

extern "C" int dtk_batch_pieces_host(dtk_batch *b, dtk_piece_view *o) {
  return !b || !o ? DTK_E_ARG : wp_finish(b, true, o);
}

extern "C" int dtk_batch_set_encode(dtk_batch *b, const dtk_encode_spec *spec, int rows_home) {
  if (!b) return DTK_E_ARG;
  DtkEncRule rule{};
  if (spec && !enc_rule_of(spec, &rule)) return DTK_E_ARG;
  const int rc = b->enc.wait();
  if (rc != DTK_OK) return rc;
  // (the finished run, if any, is encoded anew under the new spec when its rows are asked for)
  b->enc.new_run();
  b->enc_on = spec != nullptr;
  b->enc_rule = rule;
  b->enc_home = spec && rows_home != 0;
  return DTK_OK;
}

extern "C" int dtk_batch_encoded_device(dtk_batch *b, dtk_encode_view *o) {
  return !b || !o ? DTK_E_ARG : enc_finish(b, false, o);
}

extern "C" int dtk_batch_encoded_host(dtk_batch *b, dtk_encode_view *o) {
  return !b || !o ? DTK_E_ARG : enc_finish(b, true, o);
}
