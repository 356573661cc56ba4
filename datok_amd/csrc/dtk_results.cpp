// dtk_results.cpp -- a finished run's results: the device view, the copies to the host (inside the run, k_to_host,
// or on the download stream), the host view, and rendering.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <vector>

#define DTK_BLK_DECODER  // (this unit emits dtk_blk_start / dtk_blk_end of datok_gpu.h as exported functions)
#include "dtk_host.h"

namespace {
// An array that can go to the host: `count` >= 0: totals[count] elements of `size` bytes, in a device array of `cap`
// elements -- 0 tokens, 1 sentence ints, 2 texts, 3 (kPerBlock) blocks of 64 tokens, i.e. one element per 64 tokens,
// rounded up, 4 (kPerEvent) rows of the event list the copies are sized for; < 0: `size` bytes.
struct HostArray {
  uint32_t field;  // DTK_R_*
  int slot;        // dtk_batch::PB_*: its page-locked buffer
  const void *src;
  uint64_t size;
  int count;
  uint64_t cap;
  void (*view)(dtk_result_view *o, const void *p);  // where dtk_batch_result_host shows it
};
#define VIEW(f) [](dtk_result_view *o, const void *p) { o->f = static_cast<decltype(o->f)>(p); }
// (Only the download stream's copies use kPerBlock: launch_to_host masks the fields with DTK_R_ALL, which holds no
// blocked field, so the kind never reaches k_to_host -- where totals[3] would be DtkTotalsDev::n_flagged.)
constexpr int kPerBlock = 3;
constexpr int kPerEvent = 4;  // (DTK_R_EVENT_LIST is no part of DTK_R_ALL either)
static_assert(DTK_EVL_SEOT == DTK_EVL_K_SEOT && DTK_EVL_TEOT == DTK_EVL_K_TEOT && DTK_EVL_SEPS == DTK_EVL_K_SEPS,
              "the kernels' kind bits are the header's");
constexpr uint32_t kBlkFields = DTK_R_TOK_RUNE_BLK | DTK_R_TOK_BYTE_BLK;
constexpr uint32_t kBlkField[2] = {DTK_R_TOK_RUNE_BLK, DTK_R_TOK_BYTE_BLK};
constexpr uint32_t kBlkWide[2] = {DTK_R_TOK_RUNE, DTK_R_TOK_BYTE};  // what stands in for a pair that does not fit

// The batch's arrays, in the order their copies are enqueued: the large ones first (k_to_host deals its pieces out to
// its waves by array; on the download stream the small copies ride behind the large ones).
std::array<HostArray, dtk_batch::PB_N> host_arrays(const dtk_batch *b) {
  const uint64_t nd = b->n_docs;
  const HostArray t[] = {
      {DTK_R_TOK_RUNE16, dtk_batch::PB_R16, b->d_r16, 4, 0, b->d_r16.cap, VIEW(tok_r16)},
      {DTK_R_TOK_RUNE_BLK, dtk_batch::PB_RBLK, b->blk[0].d_words, 4, 0, b->blk[0].cap, VIEW(tok_rblk)},
      {DTK_R_TOK_RUNE_BLK, dtk_batch::PB_RBLK_HEAD, b->blk[0].d_heads, sizeof(dtk_off_block), kPerBlock,
       blocks_of(b->blk[0].cap), VIEW(tok_rblk_head)},
      {DTK_R_TOK_BYTE_BLK, dtk_batch::PB_BBLK, b->blk[1].d_words, 4, 0, b->blk[1].cap, VIEW(tok_bblk)},
      {DTK_R_TOK_BYTE_BLK, dtk_batch::PB_BBLK_HEAD, b->blk[1].d_heads, sizeof(dtk_off_block), kPerBlock,
       blocks_of(b->blk[1].cap), VIEW(tok_bblk_head)},
      {DTK_R_TOK_RUNE, dtk_batch::PB_RSTART, b->d_rstart, 4, 0, b->tok_cap, VIEW(tok_rstart)},
      {DTK_R_TOK_RUNE, dtk_batch::PB_REND, b->d_rend, 4, 0, b->tok_cap, VIEW(tok_rend)},
      {DTK_R_TOK_BYTE, dtk_batch::PB_BSTART, b->d_bstart, 4, 0, b->tok_cap, VIEW(tok_bstart)},
      {DTK_R_TOK_BYTE, dtk_batch::PB_BEND, b->d_bend, 4, 0, b->tok_cap, VIEW(tok_bend)},
      {DTK_R_EVENTS, dtk_batch::PB_BITS, b->d_bits, (uint64_t)EVB_KINDS * b->bit_words * 4, -1, 0, VIEW(ev_bits)},
      {DTK_R_EVENT_LIST, dtk_batch::PB_EVL_POS, b->d_evl_pos, 4, kPerEvent, b->d_evl_pos.cap, VIEW(evl_pos)},
      {DTK_R_EVENT_LIST, dtk_batch::PB_EVL_KIND, b->d_evl_kind, 1, kPerEvent, b->d_evl_kind.cap, VIEW(evl_kind)},
      {DTK_R_EVENT_LIST, dtk_batch::PB_EVL_OFF, b->d_evl_off, (nd + 1) * 4, -1, 0, VIEW(evl_off)},
      {DTK_R_EVENTS | DTK_R_EVENT_LIST, dtk_batch::PB_TAIL, b->d_doc_tail, nd * 4, -1, 0, VIEW(doc_tail)},  // (with either)
      {DTK_R_SENT, dtk_batch::PB_SENT, b->d_sent, 4, 1, b->sent_cap, VIEW(sent)},
      {DTK_R_TEXTS, dtk_batch::PB_TTOK, b->d_ttok, 4, 2, b->text_cap, VIEW(text_tok_end)},
      {DTK_R_TEXTS, dtk_batch::PB_TSENT, b->d_tsent, 4, 2, b->text_cap, VIEW(text_sent_end)},
      // (tok_off | sent_off | text_off lie back to back: dtk_batch_run)
      {DTK_R_CSR, dtk_batch::PB_CSR, b->d_csr, 3 * (nd + 1) * 8, -1, 0, VIEW(tok_off)},
      {DTK_R_STATUS, dtk_batch::PB_STATUS, b->d_status, nd * 4, -1, 0, VIEW(status)}};
  static_assert(sizeof t / sizeof t[0] == dtk_batch::PB_N, "one row per page-locked buffer");
  std::array<HostArray, dtk_batch::PB_N> r;
  std::copy(t, t + dtk_batch::PB_N, r.begin());
  return r;
}

// The blocked form of the pairs in `want` (kBlkFields), packed on the download stream itself, in front of its copies:
// the batch's stream is idle (finish()) and stays free.  The device arrays follow tok_cap like d_r16.
int pack_blocked(dtk_batch *b, uint32_t want, uint64_t n_tokens) {
  if (!b->h_blk_flag.p) {
    int rc;
    if ((rc = b->d_blk_flag.fit(2, 2)) || (rc = b->h_blk_flag.fit(2 * sizeof(uint32_t), 2 * sizeof(uint32_t)))) return rc;
    memset(b->h_blk_flag.p, 0, 2 * sizeof(uint32_t));
  }
  const int32_t *src[2][2] = {{b->d_rstart, b->d_rend}, {(const int32_t *)b->d_bstart.p, (const int32_t *)b->d_bend.p}};
  DtkPackBlkArgs a{};
  for (int k = 0; k < 2; k++) {
    if (!(want & kBlkField[k])) continue;
    dtk_batch::BlkPair &p = b->blk[k];
    if (p.cap < b->tok_cap || !p.d_words) {
      const uint64_t cap = std::max<uint64_t>(b->tok_cap, 64);
      int rc;
      p.cap = 0;
      if ((rc = p.d_words.fit(cap, cap)) || (rc = p.d_heads.fit(blocks_of(cap), blocks_of(cap)))) return rc;
      p.cap = cap;
    }
    if (n_tokens > p.cap) return DTK_E_CAPACITY;  // (finish() has grown tok_cap to the run's tokens: never expected)
    // the flag word is cleared in front of the kernel and goes home behind the blocked arrays (dtk_batch_download_begin)
    HIP_TRY(hipMemsetAsync(b->d_blk_flag + k, 0, sizeof(uint32_t), b->dl_stream));
    a.pair[a.n_pairs++] = DtkPackBlkPair{src[k][0], src[k][1], p.d_words, p.d_heads, b->d_blk_flag + k};
  }
  a.n = n_tokens;
  a.span = g_dbg.blk_span > 0 ? (uint32_t)g_dbg.blk_span : 65535u;
  if (dtk_launch_pack_blk(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "pack blocked offsets");
  return DTK_OK;
}

// DTK_R_EVENT_LIST: the list of the last run's bitmaps, compacted on the download stream in front of its copies like
// the blocked offsets.  `rows`: what the device arrays must hold and the copies will bring -- the kernels write
// nothing if the list is longer, and the count word, which goes home behind the arrays, says so.
int pack_event_list(dtk_batch *b, uint64_t rows) {
  const uint64_t n_bits = b->total + b->n_docs;
  if (n_bits > 0xFFFFFFFFull || rows > 0xFFFFFFFFull) return DTK_E_CAPACITY;
  int rc;
  if (!b->h_evl_cnt.p) {
    if ((rc = b->d_evl_cnt.fit(1, 1)) || (rc = b->h_evl_cnt.fit(sizeof(uint32_t), sizeof(uint32_t)))) return rc;
    *b->h_evl_cnt.as<uint32_t>() = 0;
  }
  const uint64_t cap = std::max<uint64_t>(rows + rows / 8, 64);
  const uint32_t tiles = dtk_evlist_tiles(n_bits, b->bit_words);
  if ((rc = b->d_evl_pos.fit(rows, cap)) || (rc = b->d_evl_kind.fit(rows, cap)) || (rc = b->d_evl_bit.fit(rows, cap)) ||
      (rc = b->d_evl_off.fit((uint64_t)b->n_docs + 1, std::max<uint64_t>((uint64_t)b->max_docs, b->n_docs) + 1)) ||
      (rc = b->d_evl_tiles.fit(tiles, std::max<uint64_t>(tiles + tiles / 8, 16))))
    return rc;
  DtkEvListArgs a{};
  a.bits = b->d_bits; a.bit_words = b->bit_words; a.n_docs = b->n_docs; a.doc_off = b->d_off; a.n_bits = n_bits;
  a.n_tiles = tiles; a.cap = (uint32_t)rows;
  a.tile_base = b->d_evl_tiles; a.count = b->d_evl_cnt; a.evl_off = b->d_evl_off;
  a.evl_pos = b->d_evl_pos; a.evl_kind = b->d_evl_kind; a.evl_bit = b->d_evl_bit;
  if (dtk_launch_evlist(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "pack event list");
  b->evl_copied = rows;
  return DTK_OK;
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
  o->n_sen = b->sen_n;
  o->sen_off = L.in(block, L.off);
  o->sen_tok_end = L.in(block, L.tok_end); o->sen_bstart = L.in(block, L.bstart); o->sen_bend = L.in(block, L.bend);
  o->sen_rstart = runes ? L.in(block, L.rstart) : nullptr; o->sen_rend = runes ? L.in(block, L.rend) : nullptr;
  o->text_sen_end = L.in(block, L.tse);
}

// Enqueues on the download stream what is still missing of: the table's kernels, and the copy of the whole block
// (home) or of its count word.  The run is complete (finish()).
int sen_enqueue(dtk_batch *b, bool home) {
  if (b->last_flags & DTK_NO_BYTE_OFFSETS) return DTK_E_STATE;  // the table is keyed on tok_bend
  const uint64_t n_bits = b->total + b->n_docs;
  // every row is an int the writer's Token closure pushes to sent[]: n_sent bounds the rows of regular documents, and
  // the count word backs the bound up (sen_finish)
  uint64_t rows = g_dbg.sen_cap >= 0 ? (uint64_t)g_dbg.sen_cap : b->totals.n_sent;
  rows = std::max<uint64_t>(std::max(rows, b->sen_need), 1);
  if (n_bits > 0xFFFFFFFFull || rows > 0xFFFFFFFFull) return DTK_E_CAPACITY;
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  int rc;
  if (b->sen_done && (b->sen_home || !home)) return DTK_OK;  // nothing is missing
  dtk_batch::Sen &L = b->sen;
  if (!b->sen_built || (!b->sen_done && rows > L.cap(L.tok_end))) {
    const uint32_t tiles = dtk_sentences_tiles(n_bits, b->bit_words);
    const uint64_t ws = 3 * rows + 2 * (uint64_t)tiles;
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
    b->sen_built = true;
    b->sen_gen++;
    b->sen_home = b->sen_done = false;
  } else if (b->sen_home) {
    return DTK_OK;  // on its way
  }
  if (home) HIP_TRY(hipMemcpyAsync(L.h.p, L.d.p, (size_t)L.bytes, hipMemcpyDeviceToHost, b->dl_stream));
  else HIP_TRY(hipMemcpyAsync(L.host(L.cnt), L.dev(L.cnt), sizeof(uint32_t), hipMemcpyDeviceToHost, b->dl_stream));
  b->sen_home = home;
  if ((rc = b->ev_sen.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev_sen, b->dl_stream));
  b->sen_waited = false;
  return DTK_OK;
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
  rows.reserve((size_t)b->sen_n);
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
  b->sen_n = n;
  b->sen_gen++;
  return DTK_OK;
}

// The table, complete: on the device, and (home) in the page-locked block.
int sen_finish(dtk_batch *b, bool home) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if (!b->h_exact_ids.empty()) home = true;  // (the splice works on the host copy)
  for (;;) {
    if ((rc = sen_enqueue(b, home)) != DTK_OK) return rc;
    if (!b->sen_waited) { HIP_TRY(hipEventSynchronize(b->ev_sen)); b->sen_waited = true; }
    if (b->sen_done) return DTK_OK;  // (the count was looked at before: this call only brought the block home)
    const uint64_t n = *b->sen.host(b->sen.cnt);
    if (n <= b->sen.cap(b->sen.tok_end)) { b->sen_n = n; break; }
    // more rows than the bound (not expected of regular documents): the kernels wrote nothing; again, for n rows
    b->sen_need = n;
    b->sen_built = false;
  }
  if (!b->h_exact_ids.empty() && (rc = sen_splice_exact(b)) != DTK_OK) return rc;
  b->sen_done = true;
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
  int rc;
  if (!b->ids_built) {
    L.clear();
    L.add(L.cnt, 1); L.add(L.id, nt);
    if ((rc = L.fit()) != DTK_OK) return rc;
    HIP_TRY(hipMemsetAsync(L.dev(L.cnt), 0, sizeof(uint64_t), b->dl_stream));
    DtkTokenIdArgs a{};
    a.text = b->d_text; a.total = b->total; a.doc_off = b->d_off; a.n_docs = b->n_docs;
    a.tok_off = b->d_tok_off; a.tok_bstart = b->d_bstart; a.tok_bend = b->d_bend; a.n_tok = nt;
    if (b->n_invalid) { const DtkSym s = sym_of(b); a.sym_base = s.base; a.sym_lut = s.lut; }
    a.vocab = b->vocab->dev;
    a.tok_id = L.dev(L.id);
    a.n_unknown = reinterpret_cast<unsigned long long *>(L.dev(L.cnt));
    a.tally = b->tally ? b->tally->d_counts.p : nullptr;
    if (dtk_launch_token_ids(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "token ids");
    b->ids_built = true;
    L.bring(L.cnt, 1);
  }
  if (home) L.bring(L.id, nt);
  if (L.pending.empty()) return DTK_OK;
  if ((rc = L.issue(b->dl_stream)) != DTK_OK || (rc = b->ev_ids.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev_ids, b->dl_stream));
  b->ids_waited = false;
  return DTK_OK;
}

// The ids, complete: on the device, and (home) in the page-locked block.
int ids_finish(dtk_batch *b, bool home, dtk_token_id_view *o) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if ((rc = ids_enqueue(b, home || b->ids_home)) != DTK_OK || (rc = ids_wait(b)) != DTK_OK) return rc;
  const dtk_batch::Ids &L = b->ids;
  o->n_tok = b->totals.n_tokens;
  o->n_unknown = *L.host(L.cnt);
  o->tok_id = L.in(home ? L.h.p : static_cast<void *>(L.d.p), L.id);
  return DTK_OK;
}

// ---- dtk_batch_set_wordpiece: the tokens' pieces (dtk_wordpiece.hip; the definition is in include/datok_gpu.h)

// Pieces the first block of a run holds: the count is known only behind the split, and nothing here waits for it.
// Running text splits few of its tokens, so half as many pieces again as tokens; a run that needs more says so
// (wp_need) and is split again into a block of that size -- which the batch's later runs start with, so a pipeline's
// slices of one kind of text pay for the second split once per slot.
uint64_t wp_cap_of(const dtk_batch *b) {
  const uint64_t nt = b->totals.n_tokens;
  return std::max(b->wp_need, nt + nt / 2 + 64);
}

// Enqueues on the download stream what is still missing of: the split (once per run and block), the copy of the two
// counters, and (home) the copies of piece_off and of the pieces -- as many as there are tokens, the rest follows
// when the count is known (wp_finish).
int wp_enqueue(dtk_batch *b, bool home) {
  if (!b->wp_vocab || (b->last_flags & DTK_NO_BYTE_OFFSETS)) return DTK_E_STATE;  // (the keys are cut out with tok_bstart / tok_bend)
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  dtk_batch::Pieces &L = b->pieces;
  const uint64_t nt = b->totals.n_tokens;
  int rc;
  if (!b->wp_built) {
    const uint64_t tiles = dtk_wp_tiles(nt);
    b->wp_cap = wp_cap_of(b);
    L.clear();
    L.add(L.cnt, 2); L.add(L.off, nt + 1); L.add(L.id, b->wp_cap); L.add(L.bend, b->wp_cap);
    if ((rc = L.fit()) != DTK_OK || (rc = b->d_wp_ws.fit(tiles + 1 + nt, tiles + 1 + nt + nt / 8)) != DTK_OK) return rc;
    HIP_TRY(hipMemsetAsync(L.dev(L.cnt), 0, 2 * sizeof(uint64_t), b->dl_stream));
    DtkWordPieceArgs a{};
    a.text = b->d_text; a.total = b->total; a.doc_off = b->d_off; a.n_docs = b->n_docs;
    a.tok_off = b->d_tok_off; a.tok_bstart = b->d_bstart; a.tok_bend = b->d_bend; a.n_tok = nt;
    if (b->n_invalid) { const DtkSym s = sym_of(b); a.sym_base = s.base; a.sym_lut = s.lut; }
    a.vocab = b->wp_vocab->dev;
    a.rule = b->wp_rule;
    a.tile_base = b->d_wp_ws.p;
    a.first = reinterpret_cast<DtkWpFirst *>(b->d_wp_ws.p + tiles + 1);
    a.cnt = reinterpret_cast<unsigned long long *>(L.dev(L.cnt));
    a.piece_off = L.dev(L.off); a.piece_id = L.dev(L.id); a.piece_bend = L.dev(L.bend);
    a.cap = b->wp_cap;
    if (dtk_launch_wordpiece(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "wordpiece");
    b->wp_built = true;
    b->wp_gen++;
    L.bring(L.cnt, 2);
  }
  // (The first copies bring nt ids and ends whatever the count turns out to be: with fewer pieces -- tokens of an empty
  //  key -- or a run that overflowed the block and wrote none, device memory nobody wrote comes home behind them.  No
  //  view shows it: n_pieces bounds every view, and an overflowed run is split and copied again.)
  if (home) { L.bring(L.off, nt + 1); L.bring(L.id, nt); L.bring(L.bend, nt); }
  if (L.pending.empty()) return DTK_OK;
  if ((rc = L.issue(b->dl_stream)) != DTK_OK || (rc = b->ev_wp.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev_wp, b->dl_stream));
  b->wp_waited = false;
  return DTK_OK;
}

// The pieces, complete: on the device, and (home, or pieces_home) in the page-locked block.  The view's pointers are
// the caller's choice alone: device pointers for home == false, whatever has been brought home beside them.
int wp_finish(dtk_batch *b, bool home, dtk_piece_view *o) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  const bool copies = home || b->wp_home;
  dtk_batch::Pieces &L = b->pieces;
  for (int round = 0;; round++) {
    if ((rc = wp_enqueue(b, copies)) != DTK_OK || (rc = wp_wait(b)) != DTK_OK) return rc;
    const uint64_t np = L.host(L.cnt)[0];
    if (np <= b->wp_cap) break;
    if (round) return DTK_E_STATE;  // (the same run's count cannot have grown)
    b->wp_need = np;                // no piece was written: once more, into a block that holds them
    b->wp_built = false;
  }
  const uint64_t np = L.host(L.cnt)[0];
  if (copies) {  // (what the first copies left out)
    L.bring(L.id, np); L.bring(L.bend, np);
    if ((rc = wp_enqueue(b, true)) != DTK_OK || (rc = wp_wait(b)) != DTK_OK) return rc;
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
  int rc;
  if ((rc = wp_enqueue(b, b->wp_home)) != DTK_OK) return rc;
  if (sentences) {
    // documents the exact pass walked get their rows on the host (sen_splice_exact): the encode waits until somebody
    // asks for it
    if (!b->h_exact_ids.empty() && !b->sen_done) return DTK_OK;
    if (!b->sen_built && (rc = sen_enqueue(b, false)) != DTK_OK) return rc;
  }
  dtk_batch::Enc &L = b->enc;
  bool issued = false;
  if (b->enc_built && (b->enc_wp_gen != b->wp_gen || (sentences && b->enc_sen_gen != b->sen_gen))) b->enc_built = false;
  if (!b->enc_built) {
    const uint64_t units_cap = sentences ? b->sen.cap(b->sen.tok_end) : b->n_docs;
    uint64_t rows = units_cap + ((R.flags & DTK_ENC_FIRST_WINDOW) ? 0u : b->wp_cap / R.step);
    rows = (std::max<uint64_t>(std::max(rows, b->enc_need), 1) + 3u) & ~3ull;  // (whole 16 bytes of ids: word_id stays aligned)
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
      a.sen_off = b->sen.dev(b->sen.off); a.sen_tok_end = b->sen.dev(b->sen.tok_end); a.sen_count = b->sen.dev(b->sen.cnt);
      a.sen_cap = units_cap;
    }
    a.piece_off = b->pieces.dev(b->pieces.off); a.piece_id = b->pieces.dev(b->pieces.id); a.piece_cap = b->wp_cap;
    a.units_cap = units_cap; a.rows_cap = rows;
    a.tile_base = b->d_enc_ws.p;
    a.unit = reinterpret_cast<DtkEncUnit *>(b->d_enc_ws.p + tiles + 1);
    a.cnt = reinterpret_cast<unsigned long long *>(b->d_enc_cnt.p);
    a.unit_row_off = L.dev(L.off); a.input_ids = L.dev(L.ids); a.row_len = L.dev(L.len); a.row_piece0 = L.dev(L.piece0);
    a.word_id = words ? L.dev(L.word) : nullptr;
    if (dtk_launch_encode(&a, b->dl_stream)) return hip_fail(hipGetLastError(), "encode");
    b->enc_built = true;
    b->enc_rows_cap = rows;
    b->enc_wp_gen = b->wp_gen; b->enc_sen_gen = b->sen_gen;
    HIP_TRY(hipMemcpyAsync(b->h_enc_cnt.p, b->d_enc_cnt.p, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, b->dl_stream));
    issued = true;
  }
  if (home) {
    // (as with the pieces: rows nobody wrote may come home behind the written ones, and no view shows them)
    if ((rc = L.h.fit((size_t)L.bytes)) != DTK_OK) return rc;
    const uint64_t first = std::min(L.cap(L.off) - 1, b->enc_rows_cap);
    L.bring(L.ids, first * R.max_len); L.bring(L.word, first * R.max_len); L.bring(L.piece0, first);
    L.bring(L.off, L.cap(L.off)); L.bring(L.len, first);
  }
  if (!L.pending.empty()) {
    if ((rc = L.issue(b->dl_stream)) != DTK_OK) return rc;
    issued = true;
  }
  if (!issued) return DTK_OK;
  if ((rc = b->ev_enc.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev_enc, b->dl_stream));
  b->enc_waited = false;
  return DTK_OK;
}

// The rows, complete: on the device, and (home, or rows_home) in the page-locked block.  The pieces and the sentence
// table are completed first; an encode that read an earlier state of either, or outgrew its block, is done again.
int enc_finish(dtk_batch *b, bool home, dtk_encode_view *o) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if (!enc_state(b)) return DTK_E_STATE;
  if ((rc = enc_wait(b)) != DTK_OK) return rc;  // (nothing reads the tables while they are made anew)
  dtk_piece_view pieces;
  if ((rc = wp_finish(b, false, &pieces)) != DTK_OK) return rc;
  const DtkEncRule &R = b->enc_rule;
  if (R.unit == DTK_ENC_SENTENCE && (rc = sen_finish(b, false)) != DTK_OK) return rc;
  const bool copies = home || b->enc_home;
  dtk_batch::Enc &L = b->enc;
  const uint64_t *cnt = nullptr;
  for (int round = 0;; round++) {
    if ((rc = enc_enqueue(b, copies)) != DTK_OK || (rc = enc_wait(b)) != DTK_OK) return rc;
    cnt = b->h_enc_cnt.as<uint64_t>();
    if (cnt[3]) break;
    if (round) return DTK_E_STATE;  // (the same run's count cannot have grown)
    b->enc_need = cnt[0];           // no row was written: once more, into a block that holds them
    b->enc_built = false;
  }
  const uint64_t n_rows = cnt[0], n_units = cnt[2];
  if (copies) {  // (what the first copies left out)
    L.bring(L.ids, n_rows * R.max_len); L.bring(L.word, n_rows * R.max_len); L.bring(L.piece0, n_rows);
    L.bring(L.off, n_units + 1); L.bring(L.len, n_rows);
    if ((rc = enc_enqueue(b, true)) != DTK_OK || (rc = enc_wait(b)) != DTK_OK) return rc;
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

int enc_wait(dtk_batch *b) {
  if (b->enc_waited) return DTK_OK;
  HIP_TRY(hipEventSynchronize(b->ev_enc));
  b->enc_waited = true;
  b->enc.landed();
  return DTK_OK;
}

extern "C" int dtk_batch_set_encode(dtk_batch *b, const dtk_encode_spec *spec, int rows_home) {
  if (!b) return DTK_E_ARG;
  DtkEncRule rule{};
  if (spec && !enc_rule_of(spec, &rule)) return DTK_E_ARG;
  const int rc = enc_wait(b);
  if (rc != DTK_OK) return rc;
  // (the finished run, if any, is encoded anew under the new spec when its rows are asked for)
  b->enc_built = false; b->enc_need = 0;
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

int wp_wait(dtk_batch *b) {
  if (b->wp_waited) return DTK_OK;
  HIP_TRY(hipEventSynchronize(b->ev_wp));
  b->wp_waited = true;
  b->pieces.landed();
  return DTK_OK;
}

extern "C" int dtk_batch_set_wordpiece(dtk_batch *b, const dtk_vocab *v, const uint8_t *prefix, uint32_t prefix_len,
                                       int32_t unk_id, uint32_t max_runes, int pieces_home) {
  if (!b || (v && v->device != b->device)) return DTK_E_ARG;
  DtkWpRule rule{};
  int rc = v ? wordpiece_rule(v->n_words, prefix, prefix_len, unk_id, max_runes, &rule) : DTK_OK;
  if (rc != DTK_OK || (rc = wp_wait(b)) != DTK_OK) return rc;  // (a split under way reads the vocabulary that was attached)
  // (the finished run, if any, is split anew under the new rule when its pieces are asked for)
  b->wp_built = false;
  b->wp_vocab = v; b->wp_rule = rule; b->wp_home = v && pieces_home != 0;
  return DTK_OK;
}

extern "C" int dtk_batch_pieces_device(dtk_batch *b, dtk_piece_view *o) {
  return !b || !o ? DTK_E_ARG : wp_finish(b, false, o);
}

extern "C" int dtk_batch_pieces_host(dtk_batch *b, dtk_piece_view *o) {
  return !b || !o ? DTK_E_ARG : wp_finish(b, true, o);
}

int ids_wait(dtk_batch *b) {
  if (b->ids_waited) return DTK_OK;
  HIP_TRY(hipEventSynchronize(b->ev_ids));
  b->ids_waited = true;
  b->ids.landed();
  return DTK_OK;
}

extern "C" int dtk_batch_set_vocab(dtk_batch *b, const dtk_vocab *v, dtk_tally *t, int ids_home) {
  if (!b || (!v && t)) return DTK_E_ARG;
  if (v && (v->device != b->device || (t && (t->device != b->device || t->n_words != v->n_words)))) return DTK_E_ARG;
  const int rc = ids_wait(b);  // (a lookup under way reads the vocabulary that was attached)
  if (rc != DTK_OK) return rc;
  // (another vocabulary: the finished run, if any, is looked up anew when its ids are asked for; the same one again
  //  keeps what was computed, so a run's tokens reach a tally once)
  if (v != b->vocab) b->ids_built = false;
  b->vocab = v; b->tally = t; b->ids_home = v && ids_home != 0;
  return DTK_OK;
}

extern "C" int dtk_batch_token_ids_device(dtk_batch *b, dtk_token_id_view *o) {
  return !b || !o ? DTK_E_ARG : ids_finish(b, false, o);
}

extern "C" int dtk_batch_token_ids_host(dtk_batch *b, dtk_token_id_view *o) {
  return !b || !o ? DTK_E_ARG : ids_finish(b, true, o);
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

extern "C" int dtk_batch_result_device(dtk_batch *b, dtk_result_view *o) {
  if (!b || !o) return DTK_E_ARG;
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  o->tok_r16 = nullptr;  // (host results only)
  o->tok_rblk = o->tok_bblk = nullptr; o->tok_rblk_head = o->tok_bblk_head = nullptr;
  o->evl_off = o->evl_pos = nullptr; o->evl_kind = nullptr;
  set_outputs(b, *o);
  o->status = b->d_status; o->ev_bits = b->d_bits; o->ev_words = b->bit_words; o->doc_tail = b->d_doc_tail;
  o->n_exact = (uint32_t)b->h_exact_ids.size();
  o->exact_doc = b->d_exact_ids; o->exact_off = b->d_exact_off; o->calls = (const dtk_call *)b->d_calls.p;
  return DTK_OK;
}

extern "C" int dtk_batch_set_result_fields(dtk_batch *b, uint32_t fields) {
  if (!b || (fields & ~(uint32_t)(DTK_R_ALL | DTK_R_TOK_RUNE16 | DTK_R_EAGER | kBlkFields | DTK_R_EVENT_LIST | DTK_R_SENTENCES))) return DTK_E_ARG;
  b->fields = fields;
  return DTK_OK;
}

// DTK_R_EAGER: the selected arrays leave for the host inside the run, by a kernel behind the compaction that reads
// the sizes where they are -- on the device (k_to_host).  Page-locked buffers sized like the device arrays; no more
// elements are copied than the device array holds (a count beyond it means the compaction wrote nothing there, and
// finish() grows the arrays and has them copied on the download stream).
int launch_to_host(dtk_batch *b) {
  const uint32_t f = b->fields & run_fields(b) & DTK_R_ALL;
  DtkToHostArgs a{};
  for (const HostArray &r : host_arrays(b)) {
    if (!(f & r.field)) continue;
    PinBuf &pb = b->pin[r.slot];
    int rc = pb.fit((size_t)(r.count >= 0 ? r.cap * r.size : r.size));
    if (rc != DTK_OK) return rc;
    void *dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp, pb.p, 0));
    a.src[a.n] = r.src; a.dst[a.n] = dp; a.bytes[a.n] = r.size; a.count_from[a.n] = r.count;
    a.cap[a.n] = r.count >= 0 ? std::min<uint64_t>(pb.cap / r.size, r.cap) : 0;
    a.n++;
  }
  if (a.n == 0) return DTK_OK;
  a.totals = &b->d_totals->n_tok;
  a.skip_if = b->last_args.skip_if;
  a.done = &b->d_totals->to_host_epoch;
  a.epoch = b->epoch;
  if (dtk_launch_to_host(&a, b->stream)) return hip_fail(hipGetLastError(), "results to the host");
  b->eager_fields = f;
  return DTK_OK;
}

// Completes the run (as dtk_batch_totals: speculation check, repairs, capacity check -- the batch's stream is idle
// afterwards) and enqueues the copies of the selected result arrays on the download stream.  Returns at once.
extern "C" int dtk_batch_set_download_stream(dtk_batch *b, void *stream) {
  if (!b) return DTK_E_ARG;
  if (b->dl_begun && !b->dl_waited) { HIP_TRY(hipEventSynchronize(b->ev_dl)); b->dl_waited = true; }
  return b->dl_stream.lend((hipStream_t)stream);
}

extern "C" void *dtk_batch_download_stream(dtk_batch *b) {
  if (!b) return nullptr;
  if (!b->dl_stream && b->dl_stream.create() != DTK_OK) return nullptr;
  return (void *)b->dl_stream;
}

extern "C" int dtk_batch_download_begin(dtk_batch *b) {
  if (!b) return DTK_E_ARG;
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  // the tokens' ids (dtk_batch_set_vocab): no result field, they ride in front of the fields' copies
  if (b->vocab && !(b->last_flags & DTK_NO_BYTE_OFFSETS) && (rc = ids_enqueue(b, b->ids_home)) != DTK_OK) return rc;
  // ... and their pieces (dtk_batch_set_wordpiece), the same way
  if (b->wp_vocab && !(b->last_flags & DTK_NO_BYTE_OFFSETS) && (rc = wp_enqueue(b, b->wp_home)) != DTK_OK) return rc;
  // ... and the model input rows made of them (dtk_batch_set_encode)
  if (enc_state(b) && (rc = enc_enqueue(b, b->enc_home)) != DTK_OK) return rc;
  uint32_t sel = b->fields & (DTK_R_ALL | DTK_R_TOK_RUNE16 | kBlkFields | DTK_R_EVENT_LIST | DTK_R_SENTENCES);
  if (sel & DTK_R_TOK_RUNE16) {
    // the narrow form holds every offset of a document of at most 32 767 bytes; a batch with a longer one gets the
    // 32-bit arrays in its place
    if (!b->max_doc_valid) {
      uint64_t m = 0;
      for (uint32_t d = 0; d < b->n_docs; d++) m = std::max(m, b->h_doc_off[d + 1] - b->h_doc_off[d]);
      b->max_doc_bytes = m;
      b->max_doc_valid = true;
    }
    // (with DTK_R_TOK_RUNE_BLK beside it the narrowest form that applies is asked for: tok_r16, else the blocks)
    if (b->max_doc_bytes <= 32767u) sel &= ~(uint32_t)DTK_R_TOK_RUNE_BLK;
    else sel = (sel & ~(uint32_t)DTK_R_TOK_RUNE16) | ((sel & DTK_R_TOK_RUNE_BLK) ? 0u : (uint32_t)DTK_R_TOK_RUNE);
  }
  // a pair whose blocks did not fit 16 bits in this run (dtk_batch_result_host saw its flag): the 32-bit arrays
  for (int k = 0; k < 2; k++)
    if (sel & b->blk_failed & kBlkField[k]) sel = (sel & ~kBlkField[k]) | kBlkWide[k];
  sel &= run_fields(b);
  if (b->dl_begun && (b->dl_fields & sel) == sel) return DTK_OK;
  const uint32_t want = sel & ~(b->dl_begun ? b->dl_fields : 0u);
  if (!dtk_batch_download_stream(b)) return hip_fail(hipGetLastError(), "download stream");
  uint64_t tot[5] = {b->totals.n_tokens, b->totals.n_sent, b->totals.n_texts, blocks_of(b->totals.n_tokens), 0};
  if (want & DTK_R_EVENT_LIST) {
    // Every SentenceEnd call appends one int (token_writer.go:108) and every TEOT is a TextEnd call: n_sent + n_texts
    // bounds the rows of regular documents, and the count word backs the bound up (dtk_batch_result_host)
    tot[kPerEvent] = g_dbg.evl_cap >= 0 ? (uint64_t)g_dbg.evl_cap : tot[1] + tot[2];
    tot[kPerEvent] = std::max(tot[kPerEvent], b->evl_need);
    if ((rc = pack_event_list(b, tot[kPerEvent])) != DTK_OK) return rc;
    // (what a slice of a stream computes from the list; behind a list packed again -- dtk_batch_result_host saw it
    //  outgrow its arrays -- it is computed again)
    if ((rc = slice_outputs(b)) != DTK_OK) return rc;
  }
  // the sentence table: its kernels and its one copy, in front of the arrays' copies (dtk_batch_sentences_host waits)
  if ((want & DTK_R_SENTENCES) && (rc = sen_enqueue(b, true)) != DTK_OK) return rc;
  const uint32_t blk_want = tot[0] ? want & kBlkFields : 0u;  // (no token: nothing to pack, empty arrays)
  if (blk_want && (rc = pack_blocked(b, blk_want, tot[0])) != DTK_OK) return rc;
  for (const HostArray &r : host_arrays(b)) {
    if (!(want & r.field)) continue;
    const uint64_t bytes = r.count >= 0 ? tot[r.count] * r.size : r.size;
    const void *src = r.src;
    if (r.field == DTK_R_TOK_RUNE16) {
      if (!bytes) continue;
      // packed on the download stream itself, in front of its copy: the batch's stream is idle (finish()) and stays free
      if ((rc = b->d_r16.fit(b->tok_cap, std::max<uint64_t>(b->tok_cap, 4))) != DTK_OK) return rc;
      if (dtk_launch_pack_r16(b->d_rstart, b->d_rend, b->d_r16, tot[0], b->dl_stream)) return hip_fail(hipGetLastError(), "pack r16");
      src = b->d_r16;
    }
    rc = b->pin[r.slot].fit((size_t)bytes);
    if (rc != DTK_OK) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(b->pin[r.slot].p, src, (size_t)bytes, hipMemcpyDeviceToHost, b->dl_stream));
  }
  for (int k = 0; k < 2; k++)
    if (blk_want & kBlkField[k])
      HIP_TRY(hipMemcpyAsync(b->h_blk_flag.as<uint32_t>() + k, b->d_blk_flag + k, sizeof(uint32_t), hipMemcpyDeviceToHost, b->dl_stream));
  b->blk_pending |= blk_want;
  if (want & DTK_R_EVENT_LIST) {
    HIP_TRY(hipMemcpyAsync(b->h_evl_cnt.p, b->d_evl_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, b->dl_stream));
    b->evl_pending = true;
  }
  if ((rc = b->ev_dl.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev_dl, b->dl_stream));
  b->dl_waited = false;
  b->dl_fields = (b->dl_begun ? b->dl_fields : 0u) | want;
  b->dl_begun = true;
  return DTK_OK;
}

extern "C" int dtk_batch_result_host(dtk_batch *b, dtk_result_view *o) {
  if (!b || !o) return DTK_E_ARG;
  int rc = dtk_batch_download_begin(b);
  if (rc != DTK_OK) return rc;
  if (!b->dl_waited) { HIP_TRY(hipEventSynchronize(b->ev_dl)); b->dl_waited = true; }
  if ((rc = ids_wait(b)) != DTK_OK) return rc;  // (a lookup that download_begin enqueued: the batch has been waited for)
  if ((rc = wp_wait(b)) != DTK_OK) return rc;   // (and a split)
  if ((rc = enc_wait(b)) != DTK_OK) return rc;  // (and an encode)
  if (b->blk_pending) {
    // A blocked pair with a block that does not fit 16 bits: its 32-bit arrays come over now and the blocked pointers
    // stay NULL.  blk_failed holds for the rest of the run: a second call neither copies again nor flips forms.
    uint32_t failed = 0;
    for (int k = 0; k < 2; k++)
      if ((b->blk_pending & kBlkField[k]) && b->h_blk_flag.as<uint32_t>()[k]) failed |= kBlkField[k];
    b->blk_pending = 0;
    if (failed) {
      b->blk_failed |= failed;
      b->dl_fields &= ~failed;
      if ((rc = dtk_batch_download_begin(b)) != DTK_OK) return rc;
      if (!b->dl_waited) { HIP_TRY(hipEventSynchronize(b->ev_dl)); b->dl_waited = true; }
    }
  }
  if (b->evl_pending) {
    // An event list longer than its copies were sized for (not expected of regular documents): the arrays grow to
    // the count, the list is packed and copied again.  evl_need holds for the rest of the run.
    b->evl_pending = false;
    const uint64_t n = *b->h_evl_cnt.as<uint32_t>();
    if (n > b->evl_copied) {
      b->evl_need = n;
      b->dl_fields &= ~(uint32_t)DTK_R_EVENT_LIST;
      if ((rc = dtk_batch_download_begin(b)) != DTK_OK) return rc;
      if (!b->dl_waited) { HIP_TRY(hipEventSynchronize(b->ev_dl)); b->dl_waited = true; }
      b->evl_pending = false;
    }
  }
  memset(o, 0, sizeof(*o));
  for (const HostArray &r : host_arrays(b))
    if (b->dl_fields & r.field) r.view(o, b->pin[r.slot].p);
  o->sent_off = o->tok_off ? o->tok_off + (b->n_docs + 1) : nullptr;
  o->text_off = o->tok_off ? o->tok_off + 2 * ((uint64_t)b->n_docs + 1) : nullptr;
  o->ev_words = b->bit_words;
  o->n_exact = (uint32_t)b->h_exact_ids.size();
  o->exact_doc = b->h_exact_ids.data(); o->exact_off = b->h_exact_off.data(); o->calls = (const dtk_call *)b->h_calls.data();
  return DTK_OK;
}

// ---------------------------------------------------------------- rendering
//
// NewTokenWriter(w, bits) for every document of the batch, on the device (dtk_render.hip).
static int render(dtk_batch *b, uint32_t bits) {
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if (bits & ~31u) return DTK_E_ARG;
  if (b->last_flags & (DTK_OFFSETS_ONLY | DTK_NO_RUNE_OFFSETS | DTK_NO_BYTE_OFFSETS)) return DTK_E_STATE;  // the run skipped what the renderer reads
  // the positions were computed under the run's NEWLINE_AFTER_EOT rule (token_writer.go:66-68)
  if ((bits ^ b->last_flags) & DTK_NEWLINE_AFTER_EOT) return DTK_E_ARG;
  bits &= 15u;
  if (b->render_flags == bits) return DTK_OK;
  hipStream_t s = b->stream;
  const uint64_t nt = b->totals.n_tokens, ns = b->totals.n_sent, nx = b->totals.n_texts, nd = b->n_docs;
  const uint64_t tt = dtk_render_tiles(nt), st = dtk_render_tiles(ns);
  const uint64_t words = 2 * (nt + 1) + (ns + 1) + 2 * tt + st + (nd + 1) + 4 * (nx + 1) + 8;
  if ((rc = b->d_rws.fit(words, words + words / 8)) != DTK_OK) return rc;
  DtkRenderArgs R{};
  R.text = b->d_text; R.doc_off = b->d_off; R.n_docs = b->n_docs; R.flags = bits;
  R.tok_off = b->d_tok_off; R.sent_off = b->d_sent_off; R.text_off = b->d_text_off;
  R.n_tok = nt; R.n_sent = ns; R.n_text = nx;
  R.rstart = b->d_rstart; R.rend = b->d_rend; R.sent = b->d_sent;
  R.bstart = b->d_bstart; R.bend = b->d_bend; R.sbefore = b->d_sbefore;
  R.ttok = b->d_ttok; R.tsent = b->d_tsent; R.ts_end = b->d_ts_end; R.doc_ns = b->d_doc_ns;
  R.sym = sym_of(b); if (!b->n_invalid) R.sym.base = nullptr;
  uint64_t *q = b->d_rws;
  R.A = q; q += nt + 1; R.P = q; q += nt + 1; R.Q = q; q += ns + 1;
  R.blkA = q; q += tt; R.blkP = q; q += tt; R.blkQ = q; q += st;
  R.ns_off = q; q += nd + 1;
  R.tx_base = q; q += nx + 1; R.tx_stream = q; q += nx + 1; R.tx_pos = q; q += nx + 1; R.tx_sent = q; q += nx + 1;
  R.out_off = b->d_out_off;
  if (dtk_launch_render(&R, 0, s)) return hip_fail(hipGetLastError(), "render sizes");
  HIP_TRY(hipMemcpyAsync(&b->h_totals->render_total, R.tx_base + nx, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t total = b->h_totals->render_total;
  if ((rc = b->d_out.fit(total, total + total / 8 + 256)) != DTK_OK) return rc;
  R.out = b->d_out; R.out_total = total;
  if (total) {
    HIP_TRY(hipMemsetAsync(b->d_out, '\n', total, s));  // every separator that is not a space
    if (dtk_launch_render(&R, 1, s)) return hip_fail(hipGetLastError(), "render bytes");
  }
  b->out_total = total;
  b->render_flags = bits;
  return DTK_OK;
}

extern "C" int dtk_batch_render_device(dtk_batch *b, uint32_t bits, dtk_render_view *o) {
  if (!b || !o) return DTK_E_ARG;
  int rc = render(b, bits);
  if (rc != DTK_OK) return rc;
  o->bytes = b->d_out; o->doc_off = b->d_out_off; o->total = b->out_total;
  return DTK_OK;
}

extern "C" int dtk_batch_render_host(dtk_batch *b, uint32_t bits, dtk_render_view *o) {
  if (!b || !o) return DTK_E_ARG;
  int rc = render(b, bits);
  if (rc != DTK_OK) return rc;
  b->h_out.resize(std::max<uint64_t>(b->out_total, 1));
  b->h_out_off.resize((size_t)b->n_docs + 1);
  if (b->out_total)
    HIP_TRY(hipMemcpyAsync(b->h_out.data(), b->d_out, b->out_total, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipMemcpyAsync(b->h_out_off.data(), b->d_out_off, ((size_t)b->n_docs + 1) * 8, hipMemcpyDeviceToHost,
                         b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  o->bytes = b->h_out.data(); o->doc_off = b->h_out_off.data(); o->total = b->out_total;
  return DTK_OK;
}

extern "C" void dtk_free(void *p) { free(p); }
