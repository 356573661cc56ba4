// dtk_batch.cpp -- the batch object: create / free, streams, input, chunking, the waits, stage timing, totals and status.
// What a run enqueues and how it is completed: dtk_run.cpp.
#include <algorithm>
#include <cstring>
#include <memory>

#include "dtk_host.h"

// The output arrays for `tok` tokens, `sent` sentence ints and `text` texts.  A group's capacity is 0 while its arrays
// are regrown: no kernel is ever handed a capacity that one of them does not have.
int alloc_outputs(dtk_batch *b, uint64_t tok, uint64_t sent, uint64_t text) {
  auto grow = [](auto &a, uint64_t n) { return a.fit(n, std::max<uint64_t>(n, 4)); };
  int rc;
  if (tok > b->tok_cap) {
    b->tok_cap = 0;
    if ((rc = grow(b->d_rstart, tok)) || (rc = grow(b->d_rend, tok)) || (rc = grow(b->d_bstart, tok)) ||
        (rc = grow(b->d_bend, tok)) || (rc = grow(b->d_sbefore, tok)))
      return rc;
    b->tok_cap = tok;
  }
  if (sent > b->sent_cap) {
    b->sent_cap = 0;
    if ((rc = grow(b->d_sent, sent))) return rc;
    b->sent_cap = sent;
  }
  if (text > b->text_cap) {
    b->text_cap = 0;
    if ((rc = grow(b->d_ttok, text)) || (rc = grow(b->d_tsent, text)) || (rc = grow(b->d_ts_end, text))) return rc;
    b->text_cap = text;
  }
  return DTK_OK;
}

extern "C" int dtk_batch_create(uint64_t max_bytes, uint32_t max_docs, dtk_batch **out) {
  if (!out || max_docs == 0) return DTK_E_ARG;
  *out = nullptr;
  if (dtk_device_count() <= 0) return DTK_E_NO_DEVICE;
  std::unique_ptr<dtk_batch> b(new dtk_batch());
  b->max_bytes = max_bytes;
  b->max_docs = max_docs;
  HIP_TRY(hipGetDevice(&b->device));
  int rc = b->stream.create();
  if (rc != DTK_OK) return rc;
  if (g_dbg.round_limit >= 0) b->round_limit = (uint32_t)g_dbg.round_limit;
  const uint64_t pad = DTK_STREAM_PAD, nd1 = (uint64_t)max_docs + 1;
  auto make = [](auto &a, uint64_t n) { return a.fit(n, n); };  // (elements, not bytes)
  if ((rc = make(b->d_text_own, max_bytes + pad)) || (rc = make(b->d_off_own, nd1)) ||
      (rc = make(b->d_sym, max_bytes + pad)) || (rc = make(b->d_rsbits, (max_bytes + pad) / 8 + 64)) ||
      // one bit per cursor position and kind: total + n_docs positions, rounded up to 16 bytes per kind, two words of slack
      (rc = make(b->d_bits, EVB_KINDS * ((max_bytes + max_docs) / 32 + 8) + 8)) ||
      // the totals block and what dtk_batch_run carves behind it: three counts, status, two check words, tail
      (rc = make(b->d_acc, DTK_TOTALS_BYTES + 3 * nd1 * 8 + 4 * (uint64_t)max_docs * 4 + 64)) ||
      (rc = make(b->d_redo, max_docs)) || (rc = make(b->d_blk_doc, max_bytes / DTK_SYM_BLOCK_BYTES + 3)) ||
      (rc = make(b->d_chunk_off, nd1)) || (rc = make(b->d_big_docs, nd1)) ||
      // the three row-offset arrays, carved from one block per run (n_docs + 1 words each, back to back: one copy brings
      // them to the host)
      (rc = make(b->d_csr, 3 * nd1)) || (rc = make(b->d_doc_ns, nd1)) ||
      (rc = make(b->d_scan_ws, ((uint64_t)max_docs / 2048 + 2) * 4)) || (rc = make(b->d_out_off, nd1)) ||
      (rc = b->h_totals_pin.fit(DTK_TOTALS_BYTES, DTK_TOTALS_BYTES)) || (rc = b->h_off_pin.fit(nd1 * 8, nd1 * 8)))
    return rc;
  b->d_tok_off = b->d_csr; b->d_sent_off = b->d_csr + nd1; b->d_text_off = b->d_csr + 2 * nd1;
  b->h_totals = b->h_totals_pin.as<DtkTotalsDev>();
  // typical German: 0.18 tokens and 0.06 sentence ints per byte; grown on demand
  rc = alloc_outputs(b.get(), max_bytes / 3 + max_docs + 16, max_bytes / 8 + 2ull * max_docs + 16,
                     max_bytes / 64 + 2ull * max_docs + 16);
  if (rc != DTK_OK) return rc;
  *out = b.release();
  return DTK_OK;
}

dtk_batch::~dtk_batch() {
  if (stream) (void)hipStreamSynchronize(stream);
  if (up_stream) (void)hipStreamSynchronize(up_stream);
  if (dl_begun && !dl_waited) (void)hipEventSynchronize(ev_dl);
  (void)derived_wait(this);
}

extern "C" void dtk_batch_free(dtk_batch *b) { delete b; }

extern "C" void *dtk_batch_stream(dtk_batch *b) { return b ? (void *)b->stream : nullptr; }

// Everything this batch has enqueued so far has finished.  With a stream of its own: the stream; on a lent stream
// (shared with other batches) only the batch's own last run, by its event.
int wait_ran(dtk_batch *b) {  // the kernels of the batch's last run (not an upload on the lent upload stream)
  if (b->stream.mine) HIP_TRY(hipStreamSynchronize(b->stream));
  else if (b->ev_ran_valid) HIP_TRY(hipEventSynchronize(b->ev_ran));
  return DTK_OK;
}
int wait_own(dtk_batch *b) {
  if (b->up_pending) { HIP_TRY(hipEventSynchronize(b->ev_up)); }
  return wait_ran(b);
}

extern "C" int dtk_batch_set_streams(dtk_batch *b, void *compute, void *upload) {
  if (!b) return DTK_E_ARG;
  int rc = wait_own(b);
  if (rc != DTK_OK) return rc;
  if (compute && (rc = b->stream.lend((hipStream_t)compute)) != DTK_OK) return rc;
  b->up_stream = (hipStream_t)upload;
  return upload ? b->ev_up.ensure(hipEventDisableTiming) : DTK_OK;
}

extern "C" int dtk_batch_set_input(dtk_batch *b, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs) {
  if (!b || !doc_off || n_docs == 0) return DTK_E_ARG;
  if (n_docs > b->max_docs) return DTK_E_CAPACITY;
  if (doc_off[0] != 0) return DTK_E_ARG;
  for (uint32_t d = 0; d < n_docs; d++) {
    if (doc_off[d + 1] < doc_off[d]) return DTK_E_ARG;
    if (doc_off[d + 1] - doc_off[d] >= 0x7FFFFFF0ull) return DTK_E_ARG;  // 31-bit cursor positions
  }
  const uint64_t total = doc_off[n_docs];
  if (total > b->max_bytes || total + n_docs + 64 >= (1ull << 32)) return DTK_E_CAPACITY;  // 32-bit position bits
  if (total && !text) return DTK_E_ARG;
  { int rc = wait_own(b); if (rc != DTK_OK) return rc; }  // the previous run may still read the buffers
  { int rc = derived_wait(b); if (rc != DTK_OK) return rc; }  // (and its derived tables on the download stream, the text)
  hipStream_t us = b->up_stream ? b->up_stream : b->stream;
  if (total) HIP_TRY(hipMemcpyAsync(b->d_text_own, text, total, hipMemcpyHostToDevice, us));
  memcpy(b->h_off_pin.p, doc_off, ((size_t)n_docs + 1) * 8);
  HIP_TRY(hipMemcpyAsync(b->d_off_own, b->h_off_pin.p, ((uint64_t)n_docs + 1) * 8, hipMemcpyHostToDevice, us));
  if (b->up_stream) { HIP_TRY(hipEventRecord(b->ev_up, us)); b->up_pending = true; }
  // the lane plan only depends on the offsets: a stream of equally shaped batches keeps it
  const bool same = b->plan_valid && b->d_off == b->d_off_own && b->n_docs == n_docs &&
                    b->h_doc_off.size() == (size_t)n_docs + 1 &&
                    memcmp(b->h_doc_off.data(), doc_off, ((size_t)n_docs + 1) * 8) == 0;
  b->d_text = b->d_text_own;
  b->d_off = b->d_off_own;
  b->n_docs = n_docs;
  b->total = total;
  b->ran = false;
  if (!same) {
    b->h_doc_off.assign(doc_off, doc_off + n_docs + 1);
    b->plan_valid = false;
    b->max_doc_valid = false;
  }
  return DTK_OK;
}

extern "C" int dtk_batch_set_input_device(dtk_batch *b, const void *d_text, const void *d_doc_off,
                                          uint32_t n_docs, uint64_t total_bytes) {
  if (!b || !d_doc_off || n_docs == 0 || (total_bytes && !d_text)) return DTK_E_ARG;
  if (n_docs > b->max_docs || total_bytes > b->max_bytes || total_bytes + n_docs + 64 >= (1ull << 32)) return DTK_E_CAPACITY;
  // lane planning needs the offsets on the host: one copy per input, not per run.  They are checked in a copy of
  // their own: a rejected call leaves the batch's input, its plan and its host offsets as they were.
  std::vector<uint64_t> off((size_t)n_docs + 1);
  HIP_TRY(hipMemcpy(off.data(), d_doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyDeviceToHost));
  { const int rc = derived_wait(b); if (rc != DTK_OK) return rc; }  // (a derived table still reads the input it belongs to)
  if (off[0] != 0 || off[n_docs] != total_bytes) return DTK_E_ARG;
  for (uint32_t d = 0; d < n_docs; d++)
    if (off[d + 1] < off[d] || off[d + 1] - off[d] >= 0x7FFFFFF0ull) return DTK_E_ARG;
  b->d_text = (const uint8_t *)d_text;
  b->d_off = (const uint64_t *)d_doc_off;
  b->n_docs = n_docs;
  b->total = total_bytes;
  b->ran = false;
  b->h_doc_off.swap(off);
  b->plan_valid = false;
  b->max_doc_valid = false;
  return DTK_OK;
}

extern "C" int dtk_batch_set_chunking(dtk_batch *b, uint32_t chunk_bytes, uint32_t warm_bytes) {
  if (!b) return DTK_E_ARG;
  if (chunk_bytes != 0 && chunk_bytes != 0xFFFFFFFFu && chunk_bytes < 16) return DTK_E_ARG;
  b->cfg_chunk = chunk_bytes;
  b->cfg_warm = warm_bytes;
  b->plan_valid = false;
  return DTK_OK;
}

extern "C" int dtk_batch_set_warm_extend(dtk_batch *b, uint32_t max_bytes) {
  if (!b) return DTK_E_ARG;
  b->cfg_extend = max_bytes > 4096u ? 4096u : max_bytes;
  return DTK_OK;
}

extern "C" int dtk_batch_set_profiling(dtk_batch *b, int enable) {
  if (!b) return DTK_E_ARG;
  if (enable)
    for (Event &e : b->ev)
      if (const int rc = e.ensure(hipEventDefault)) return rc;
  b->profiling = enable != 0;
  return DTK_OK;
}

extern "C" int dtk_batch_stage_ms(dtk_batch *b, float ms[DTK_N_STAGES]) {
  if (!b || !ms) return DTK_E_ARG;
  if (!b->ran || !b->profiling) return DTK_E_STATE;
  HIP_TRY(hipStreamSynchronize(b->stream));
  for (int i = 0; i < DTK_N_STAGES; i++) HIP_TRY(hipEventElapsedTime(&ms[i], b->ev[i], b->ev[i + 1]));
  return DTK_OK;
}

extern "C" int dtk_batch_sync(dtk_batch *b) {
  if (!b) return DTK_E_ARG;
  return wait_own(b);
}

extern "C" int dtk_batch_totals(dtk_batch *b, dtk_totals *out) {
  if (!b || !out) return DTK_E_ARG;
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  *out = b->totals;
  return DTK_OK;
}

extern "C" int dtk_batch_status_host(dtk_batch *b, uint32_t *status, uint32_t n) {
  if (!b || !status || n > b->n_docs) return DTK_E_ARG;
  int rc = finish(b);
  if (rc != DTK_OK) return rc;
  if (n) HIP_TRY(hipMemcpy(status, b->d_status, (size_t)n * 4, hipMemcpyDeviceToHost));
  return DTK_OK;
}

// Test accessor (datok_gpu.h): what k_symbolize wrote in the batch's last run, read-only and in the terms of the model
// file -- codes go through the model's code table, the device's column index back through dtk_model::col.
extern "C" int dtk_batch_debug_stream(dtk_batch *b, uint16_t *entries, uint32_t *rune_start_words, uint32_t *saw_invalid) {
  if (!b || !b->ran || !b->last_model) return DTK_E_ARG;
  { const int rc = wait_own(b); if (rc != DTK_OK) return rc; }
  const dtk_model *m = b->last_model;
  const size_t n = (size_t)b->total;
  if (entries && n) {
    if (m->sig.n_codes) {
      std::vector<uint8_t> codes(n);
      uint16_t table[256];
      HIP_TRY(hipMemcpy(codes.data(), b->d_sym.p, n, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(table, m->sig.code_entry, sizeof table, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; i++) entries[i] = table[codes[i]];
    } else {
      HIP_TRY(hipMemcpy(entries, b->d_sym.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    // column -> symbol of the file (the columns are a permutation of the symbols, layout_matrix; none: the symbol itself)
    std::vector<uint16_t> sym_of_col(DTK_SYM_MASK + 1u);
    for (uint32_t c = 0; c <= DTK_SYM_MASK; c++) sym_of_col[c] = (uint16_t)c;
    for (size_t a = 0; a < m->col.size(); a++)
      if (m->col[a] <= DTK_SYM_MASK) sym_of_col[m->col[a]] = (uint16_t)a;
    for (size_t i = 0; i < n; i++)
      entries[i] = (uint16_t)((entries[i] & ~DTK_SYM_MASK) | sym_of_col[entries[i] & DTK_SYM_MASK]);
  }
  if (rune_start_words && n)
    HIP_TRY(hipMemcpy(rune_start_words, b->d_rsbits.p, (n + 31) / 32 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (saw_invalid) {
    uint64_t seen = 0;
    HIP_TRY(hipMemcpy(&seen, &b->d_totals->invalid_epoch, sizeof seen, hipMemcpyDeviceToHost));
    *saw_invalid = (n && seen == b->epoch) ? 1u : 0u;
  }
  return DTK_OK;
}
