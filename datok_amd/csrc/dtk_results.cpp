// dtk_results.cpp -- a finished run's results: the device view, the copies to the host (inside the run, k_to_host,
// or on the download stream), the host view, and rendering.  (The tables derived from them: dtk_derived.cpp.)
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
}  // namespace

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

extern "C" int dtk_batch_set_result_fields(dtk_batch *b, uint32_t fields) {
  if (!b || (fields & ~(uint32_t)(DTK_R_ALL | DTK_R_TOK_RUNE16 | DTK_R_EAGER | kBlkFields | DTK_R_EVENT_LIST | DTK_R_SENTENCES))) return DTK_E_ARG;
  b->fields = fields;
  return DTK_OK;
}

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

// Completes the run (as dtk_batch_totals: speculation check, repairs, capacity check -- the batch's stream is idle
// afterwards) and enqueues the copies of the selected result arrays on the download stream.  Returns at once.
extern "C" int dtk_batch_download_begin(dtk_batch *b) {
  if (!b) return DTK_E_ARG;
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if ((rc = derived_enqueue(b)) != DTK_OK) return rc;  // (ids, pieces, model input rows: no result field selects them)
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
  if ((rc = derived_wait(b)) != DTK_OK) return rc;  // (what download_begin enqueued of them: the batch has been waited for)
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
  const uint64_t nx = b->totals.n_texts;
  DtkRenderArgs R{};
  R.text = b->d_text; R.doc_off = b->d_off; R.n_docs = b->n_docs; R.flags = bits;
  R.tok_off = b->d_tok_off; R.sent_off = b->d_sent_off; R.text_off = b->d_text_off;
  R.n_tok = b->totals.n_tokens; R.n_sent = b->totals.n_sent; R.n_text = nx;
  const uint64_t words = dtk_render_ws(&R, nullptr);
  if ((rc = b->d_rws.fit(words, words + words / 8)) != DTK_OK) return rc;
  (void)dtk_render_ws(&R, b->d_rws);
  R.rstart = b->d_rstart; R.rend = b->d_rend; R.sent = b->d_sent;
  R.bstart = b->d_bstart; R.bend = b->d_bend; R.sbefore = b->d_sbefore;
  R.ttok = b->d_ttok; R.tsent = b->d_tsent; R.ts_end = b->d_ts_end; R.doc_ns = b->d_doc_ns;
  R.sym = sym_of(b); if (!b->n_invalid) R.sym.base = nullptr;
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
