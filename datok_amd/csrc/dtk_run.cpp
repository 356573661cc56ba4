// dtk_run.cpp -- one run of a batch: the lane plan, what dtk_batch_run enqueues (clear, symbolise, first pass, tail) and
// what finish() does behind it (repair rounds from the host, growth, the late EOT kernel, the exact pass, the totals).
// The state that passes between runs (fields of dtk_batch, dtk_host.h):
//   a run reads, from the run before   expect_repairs (two device-side rounds), expect_eot (both compaction kernels with
//                                      the run), acc_primed (k_symbolize clears the accumulators), plan_valid (plan_lanes)
//   it leaves for its finish()         dev_rounds (chunked runs only: n_bad[dev_rounds] is the word the tail looked at),
//                                      ran_full (the EOT kernel has run), eager_fields (what k_to_host was asked for),
//                                      last_args.skip_if (the word the last compaction looked at, or null)
//   finish() leaves                    for the next run expect_repairs, expect_eot; for the readers results_changed,
//                                      n_invalid, totals_valid, and dl_begun / dl_waited / dl_fields (the eager copy counts)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dtk_host.h"

static bool is_slice(const dtk_batch *b) { return b->open_slice != 0 || b->has_carry; }  // (batch_set_slice)

// Splits the documents into chunk lanes (host side of the speculative walk).
static int plan_lanes(dtk_batch *b) {
  if (b->plan_valid) return DTK_OK;
  // The tables go to the device as asynchronous copies from one page-locked staging buffer, on the stream the input
  // was uploaded on: a pipeline of ragged slices (every slice another plan) used to wait here for the slice's upload
  // and then for eight synchronous copies, one after the other.
  { const int rc_ = wait_ran(b); if (rc_ != DTK_OK) return rc_; }  // (the previous run read the old tables)
  std::vector<uint8_t> stage;
  struct Put { void *dst; size_t at, n; };
  std::vector<Put> puts;
  auto put = [&](void *dst, const void *src, size_t n) {
    if (!n) return;
    const size_t at = (stage.size() + 15) & ~(size_t)15;
    stage.resize(at + n);
    memcpy(stage.data() + at, src, n);
    puts.push_back(Put{dst, at, n});
  };
  {
    // document of the first byte of every symbolise block (+ one entry behind the end)
    const uint64_t nblk = (b->total + DTK_SYM_BLOCK_BYTES - 1) / DTK_SYM_BLOCK_BYTES;
    std::vector<uint32_t> blk((size_t)nblk + 2);
    uint32_t d = 0;
    for (uint64_t i = 0; i <= nblk; i++) {
      const uint64_t g = i * DTK_SYM_BLOCK_BYTES;
      while (d + 1 < b->n_docs && b->h_doc_off[d + 1] <= g) d++;
      blk[i] = d;
    }
    blk[nblk + 1] = b->n_docs - 1;
    put(b->d_blk_doc, blk.data(), blk.size() * 4);
  }
  {
    // One lane per document pays for many tiny documents (tweets, single sentences): 64-byte documents compact five
    // times faster that way.  From 256 bytes on the lanes' scattered row stores cost more than a wave per document
    // (measured: 256 B 245 -> 274 us, 1 KiB 81 -> 282 us per 32 MiB), hence the low limit.
    const bool e_sm = g_dbg.small_max >= 0;
    uint32_t sm = b->n_docs >= 2048u ? 160u : 0u;
    if (e_sm) sm = (uint32_t)g_dbg.small_max;
    std::vector<uint32_t> big;
    if (sm)
      for (uint32_t d = 0; d < b->n_docs; d++)
        if (b->h_doc_off[d + 1] - b->h_doc_off[d] > sm) big.push_back(d);
    // (the lane kernel's time is a fixed 30 us of latency -- a lane's sequential loop over its document -- which only
    //  pays once it replaces 16 384 waves or more; 8192 Zipf-length documents: compaction 68 -> 98 us with it)
    if (!e_sm && b->n_docs - big.size() < 16384u) { sm = 0; big.clear(); }
    b->small_max = sm;
    b->n_big = (uint32_t)big.size();
    put(b->d_big_docs, big.data(), big.size() * 4);
  }
  uint32_t C = b->cfg_chunk;
  if (C == 0xFFFFFFFFu) {
    // enough lanes to give every SIMD of the chip a few waves, but chunks no shorter than
    // a few warm-ups: 256 CUs x 4 SIMDs x 64 lanes = 65536 lanes per "wave per SIMD"
    // measured: 128 is best for 16 MiB (131072 lanes = 2 waves per SIMD); large batches are
    // flat from 128 to 1024 and lose beyond (fewer lanes than the chip holds)
    const uint64_t want_lanes = 4ull * 65536ull;
    uint64_t c = b->total / want_lanes;
    uint32_t p2 = 128;
    while (p2 * 2 <= c && p2 < DTK_LDS_BIT_CHUNK_MAX) p2 <<= 1;  // (up to what a wave's LDS bitmaps cover)
    C = p2;
  }
  b->chunk = C;
  auto flush = [&]() -> int {
    int rc_ = b->h_plan.fit(stage.size());
    if (rc_ != DTK_OK) return rc_;
    memcpy(b->h_plan.p, stage.data(), stage.size());
    hipStream_t us = b->up_stream ? b->up_stream : b->stream;
    for (const Put &q : puts)
      HIP_TRY(hipMemcpyAsync(q.dst, (const uint8_t *)b->h_plan.p + q.at, q.n, hipMemcpyHostToDevice, us));
    if (b->up_stream) { HIP_TRY(hipEventRecord(b->ev_up, us)); b->up_pending = true; }  // (the kernels wait for this too)
    return DTK_OK;
  };
  if (C == 0) {
    b->n_lanes = 0;
    int rc_ = flush();
    if (rc_ != DTK_OK) return rc_;
    b->plan_valid = true;
    return DTK_OK;
  }
  const uint32_t nd = b->n_docs;
  std::vector<uint32_t> chunk_off((size_t)nd + 1);
  uint64_t lanes = 0;
  for (uint32_t d = 0; d < nd; d++) {
    chunk_off[d] = (uint32_t)lanes;
    const uint64_t len = b->h_doc_off[d + 1] - b->h_doc_off[d];
    lanes += len ? (len + C - 1) / C : 1;
    if (lanes >= 0x7FFFFFFFull) return DTK_E_CAPACITY;
  }
  chunk_off[nd] = (uint32_t)lanes;
  std::vector<uint32_t> lane_doc((size_t)lanes);
  for (uint32_t d = 0; d < nd; d++)
    for (uint32_t L = chunk_off[d]; L < chunk_off[d + 1]; L++) lane_doc[L] = d;
  // (a group's capacity is 0 while its arrays are regrown, and every array holds at least what it says afterwards)
  if (lanes > b->lane_cap) {
    const uint64_t cap = lanes + lanes / 8 + 64;
    int rc_;
    b->lane_cap = 0;
    if ((rc_ = b->d_lane_doc.fit(cap, cap)) || (rc_ = b->d_lane_cnt.fit(cap, cap)) || (rc_ = b->d_lane_start.fit(cap, cap)) ||
        (rc_ = b->d_lane_end.fit(cap, cap)) || (rc_ = b->d_lane_plan.fit(cap, cap)))
      return rc_;
    b->lane_cap = (uint32_t)cap;
  }
  // segments of DTK_SEG_LANES lanes: the unit of k_compact for documents with many lanes
  std::vector<uint32_t> seg_doc, seg_lane0, seg_nl, doc_seg0((size_t)nd + 1);
  b->long_docs = false;
  b->max_doc_lanes = 0;
  for (uint32_t d = 0; d < nd; d++) {
    doc_seg0[d] = (uint32_t)seg_doc.size();
    const uint32_t L0 = chunk_off[d], L1 = chunk_off[d + 1];
    if (L1 - L0 > DTK_SEG_LANES) b->long_docs = true;
    b->max_doc_lanes = std::max(b->max_doc_lanes, L1 - L0);
    for (uint32_t L = L0; L < L1; L += DTK_SEG_LANES) {
      seg_doc.push_back(d);
      seg_lane0.push_back(L);
      seg_nl.push_back(std::min<uint32_t>(DTK_SEG_LANES, L1 - L));
    }
  }
  doc_seg0[nd] = (uint32_t)seg_doc.size();
  const uint32_t ns = (uint32_t)seg_doc.size();
  if (ns > b->seg_cap) {
    const uint64_t cap = (uint64_t)ns + ns / 8 + 64, tab = 3 * cap + 2 * ((uint64_t)b->max_docs + 1);
    int rc_;
    b->seg_cap = 0;
    if ((rc_ = b->d_seg_tab.fit(tab, tab)) || (rc_ = b->d_seg_sum.fit(cap, cap)) || (rc_ = b->d_seg_in.fit(cap, cap)))
      return rc_;
    b->seg_cap = (uint32_t)cap;
  }
  b->n_segs = ns;
  put(b->d_seg_tab, seg_doc.data(), (size_t)ns * 4);
  put(b->d_seg_tab + b->seg_cap, seg_lane0.data(), (size_t)ns * 4);
  put(b->d_seg_tab + 2 * (size_t)b->seg_cap, seg_nl.data(), (size_t)ns * 4);
  put(b->d_seg_tab + 3 * (size_t)b->seg_cap, doc_seg0.data(), ((size_t)nd + 1) * 4);
  put(b->d_lane_doc, lane_doc.data(), lanes * 4);
  put(b->d_chunk_off, chunk_off.data(), ((size_t)nd + 1) * 4);
  { const int rc_ = flush(); if (rc_ != DTK_OK) return rc_; }
  b->n_lanes = (uint32_t)lanes;
  b->plan_valid = true;
  return DTK_OK;
}

// the batch's symbol stream as its last run wrote it: codes + the model's table, or 16-bit entries
DtkSym sym_of(const dtk_batch *b) {
  const dtk_model *m = b->last_model;
  return DtkSym{b->d_sym, (m && m->sig.n_codes) ? m->sig.code_entry : nullptr};
}

DtkWalkArgs walk_args(dtk_batch *b) {
  DtkWalkArgs w{};
  w.sym = sym_of(b); w.doc_off = b->d_off; w.n_docs = b->n_docs;
  w.bits = b->d_bits; w.bit_words = b->bit_words; w.doc_tail = b->d_doc_tail; w.status = b->d_status;
  w.tok_cnt = b->d_tok_cnt; w.sent_cnt = b->d_sent_cnt; w.text_cnt = b->d_text_cnt;
  w.steps = (unsigned long long *)dtk_step_stripe(b->d_totals, 0);
  w.step_factor = 2048;  // look-ahead is bounded by the 1024-rune window (matrix.go:365)
  w.init_rec = b->has_carry ? b->d_init_rec.p : nullptr;  // a slice of a stream (batch_set_slice)
  w.open_stop = b->open_slice; w.open_fin = b->d_open_fin;
  return w;
}

static DtkSpecArgs spec_args(dtk_batch *b, bool redo) {
  DtkSpecArgs s{};
  s.n_lanes = b->n_lanes; s.chunk = b->chunk; s.warm = b->cfg_warm;
  s.lane_doc = b->d_lane_doc; s.chunk_off = b->d_chunk_off;
  s.lane_start = b->d_lane_start; s.lane_end = b->d_lane_end; s.lane_plan = b->d_lane_plan;
  s.lane_cnt = b->d_lane_cnt; s.first_bad = b->d_first_bad; s.fail_lane = b->d_fail_lane;
  s.redo_from = redo ? b->d_redo : nullptr;
  s.text = b->d_text;
  s.warm_extend = b->cfg_extend;
  // the walk collects its event bits in LDS, one set of bitmaps per wave (test hook LDS_BITS=0: straight to memory)
  const bool lds = g_dbg.lds_bits != 0;
  s.lds_words = (lds && b->chunk <= DTK_LDS_BIT_CHUNK_MAX) ? DTK_LDS_BIT_WORDS(b->chunk) : 0u;
  return s;
}

// ---- a slice of one long stream (dtk_streamer.cpp)
int batch_set_slice(dtk_batch *b, uint32_t open_slice, const DtkLaneState *carry) {
  int rc;
  if ((open_slice || carry) && !b->h_init_rec.p) {
    if ((rc = b->d_init_rec.fit(1, 1)) || (rc = b->d_open_fin.fit(1, 1)) ||
        (rc = b->h_init_rec.fit(sizeof(DtkLaneState), sizeof(DtkLaneState))))
      return rc;
  }
  // (called between runs: the last run, which copied the record from h_init_rec, has been finished by its results' reader)
  b->open_slice = open_slice;
  b->has_carry = carry != nullptr;
  if (carry) *b->h_init_rec.as<DtkLaneState>() = *carry;
  return DTK_OK;
}

int batch_cut(dtk_batch *b, DtkStreamCut *out) {
  const int rc = finish(b);
  if (rc == DTK_OK) *out = b->h_totals->cut;
  return rc;
}

// the slice's document ends at its cut (dtk_streamcut.hip)
static int launch_stream_cut(dtk_batch *b, const uint32_t *skip_if) {
  DtkStreamCutArgs x{};
  x.slice = b->open_slice; x.init_rec = b->has_carry ? b->d_init_rec.p : nullptr;
  x.chunk = b->chunk; x.n_lanes = b->n_lanes;
  x.lane_start = b->d_lane_start; x.lane_cnt = b->d_lane_cnt; x.open_fin = b->d_open_fin;
  x.bits = b->d_bits; x.bit_words = b->bit_words; x.doc_tail = b->d_doc_tail; x.status = b->d_status;
  x.tok_cnt = b->d_tok_cnt; x.sent_cnt = b->d_sent_cnt; x.text_cnt = b->d_text_cnt;
  x.skip_if = skip_if; x.out = &b->d_totals->cut;
  if (dtk_launch_stream_cut(&x, b->stream)) return hip_fail(hipGetLastError(), "stream cut");
  return DTK_OK;
}

// The compaction kernels `which` names, behind the segments' carries.  What they are given comes from the batch alone, but
// for skip_if (the word to look at first, or null); b->last_args records it for launch_to_host and the launches of finish().
static int launch_compact(dtk_batch *b, DtkCompactWhich which, const uint32_t *skip_if) {
  DtkCompactArgs a{};
  a.text = b->d_text; a.rs_bits = (const uint32_t *)b->d_rsbits.p; a.doc_off = b->d_off; a.n_docs = b->n_docs;
  a.bits = b->d_bits; a.bit_words = b->bit_words; a.doc_tail = b->d_doc_tail; a.status = b->d_status;
  a.flags = b->last_flags & DTK_NEWLINE_AFTER_EOT; a.kind = b->last_model->kind;
  a.totals = &b->d_totals->n_tok; a.skip_if = skip_if;
  set_outputs(b, a);
  a.tok_cap = b->tok_cap; a.sent_cap = b->sent_cap; a.text_cap = b->text_cap;
  // a document of many lanes is compacted by one wave per DTK_SEG_LANES lanes (a double-array document
  // with an EOT inside stays sequential: k_seg_scan decides)
  const bool seg = b->chunk != 0 && b->long_docs;
  a.seg_doc = seg ? b->d_seg_tab.p : nullptr;
  a.seg_lane0 = b->d_seg_tab + b->seg_cap; a.seg_nl = b->d_seg_tab + 2 * (size_t)b->seg_cap;
  a.n_segs = b->n_segs; a.chunk_off = b->d_chunk_off; a.lane_start = b->d_lane_start; a.lane_cnt = b->d_lane_cnt;
  a.seg_sum = b->d_seg_sum; a.seg_in = b->d_seg_in;
  a.doc_seq = b->d_seg_tab + 3 * (size_t)b->seg_cap + b->max_docs + 1;
  a.any_irregular = &b->d_totals->any_irregular; a.any_eot = &b->d_totals->any_eot;
  b->last_args = a;
  if (seg && (which & DTK_COMPACT_PLAIN) && dtk_launch_seg_prepare(&a, b->d_seg_tab + 3 * (size_t)b->seg_cap, b->stream))
    return hip_fail(hipGetLastError(), "segment carries");
  if (dtk_launch_compact(&a, b->small_max, b->d_big_docs, b->n_big, which, b->stream))
    return hip_fail(hipGetLastError(), "compact pass 2");
  if (which & DTK_COMPACT_EOT) b->ran_full = true;
  return DTK_OK;
}

static int launch_spec(dtk_batch *b, const DtkWalkArgs *w, const DtkSpecArgs *sp, DtkSpecStage stage, uint32_t *n_bad, const char *what) {
  const dtk_model *m = b->last_model;
  // the sticky `ok` only matters where an arc on the unknown symbol exists (matrix.go:478-485)
  const uint32_t cmp_mask = LANE_F_SENT | LANE_F_TEXT | (m->unknown_used ? LANE_F_OK : 0u);
  if (dtk_launch_spec(&m->tab, w, sp, stage, cmp_mask, b->d_redo, n_bad, b->stream)) return hip_fail(hipGetLastError(), what);
  return DTK_OK;
}

// One repair round on the batch's stream: spread + reset, clear, then the stages of the first pass restricted to
// what is repaired; the documents still broken afterwards are counted in *n_bad_out (zero before the round).  go: a
// round enqueued ahead of time looks at that word first (DtkSpecArgs::go), null: it runs.
static int repair_round(dtk_batch *b, const DtkWalkArgs *w, const uint32_t *go, uint32_t *n_bad_out) {
  const char *what = "speculative repair";
  DtkSpecArgs sp = spec_args(b, true); sp.go = go;
  if (const int rc = launch_spec(b, w, &sp, DTK_SPEC_SPREAD_RESET, n_bad_out, what)) return rc;
  if (dtk_launch_redo_clear(w, &sp, b->stream)) return hip_fail(hipGetLastError(), what);
  for (DtkSpecStage stage : {DTK_SPEC_LINK, DTK_SPEC_WALK, DTK_SPEC_VERIFY, DTK_SPEC_FIX})
    if (const int rc = launch_spec(b, w, &sp, stage, n_bad_out, what)) return rc;
  return DTK_OK;
}

static int mark(dtk_batch *b, int i) {  // profiling: ends interval i - 1 of dtk_batch_stage_ms and begins interval i
  if (b->profiling) HIP_TRY(hipEventRecord(b->ev[i], b->stream));
  return DTK_OK;
}

static int settle_last_run(dtk_batch *b) {
  if (b->dl_begun && !b->dl_waited) { HIP_TRY(hipEventSynchronize(b->ev_dl)); b->dl_waited = true; }  // (the last run's results on their way out)
  b->dl_begun = false; b->blk_pending = b->blk_failed = 0; b->evl_pending = false; b->evl_need = 0;
  // (the last run's derived tables read the result arrays this one writes.  Each is waited for by its own event: one
  //  enqueued without a wait has ev_dl or another table's event behind it, and this does not rely on that)
  { const int rc_ = derived_wait(b); if (rc_ != DTK_OK) return rc_; }
  b->sen.new_run(); b->sen.done = false;
  b->ids.new_run();
  b->pieces.new_run(true);  // (need is kept: what a run of this batch needed, the next ones start with)
  b->enc.new_run();
  if (b->up_pending) {  // the kernels wait for the input's upload on the other stream
    HIP_TRY(hipStreamWaitEvent(b->stream, b->ev_up, 0));
    b->up_pending = false;
  }
  return DTK_OK;
}

// Carves the accumulator block for this run's document count: totals, counts, status, check words -- *acc_used bytes,
// cleared together with the event bitmaps by one launch here, or (*folded) by k_symbolize's blocks.
static int clear_accumulators(dtk_batch *b, size_t *acc_used, bool *folded) {
  const size_t nd = b->n_docs;
  uint8_t *q = b->d_acc;
  b->d_tok_off = b->d_csr; b->d_sent_off = b->d_csr + (nd + 1); b->d_text_off = b->d_csr + 2 * (nd + 1);
  b->d_totals = (DtkTotalsDev *)q; q += DTK_TOTALS_BYTES;  // (the striped lookup counters right behind the totals)
  b->d_tok_cnt = (uint64_t *)q; q += (nd + 1) * 8;
  b->d_sent_cnt = (uint64_t *)q; q += (nd + 1) * 8;
  b->d_text_cnt = (uint64_t *)q; q += (nd + 1) * 8;
  b->d_status = (uint32_t *)q; q += nd * 4;
  b->d_first_bad = (uint32_t *)q; q += nd * 4;
  b->d_fail_lane = (uint32_t *)q; q += nd * 4;
  b->d_doc_tail = (uint32_t *)q; q += nd * 4;
  *acc_used = ((size_t)(q - b->d_acc) + 15) & ~(size_t)15;  // the block has 64 bytes of slack
  b->bit_words = (uint32_t)(((b->total + nd) / 32 + 8) & ~(uint64_t)3);  // 16-byte multiples per kind
  const bool fold = b->total > 0;  // (the event bitmaps are cleared by k_symbolize's blocks, unless it does not run)
  // ... and the accumulator block too, once it has been cleared whole (invalid_epoch, which k_symbolize's own blocks
  // write, is left out there: it holds the number of the last run that saw invalid UTF-8)
  *folded = fold && b->acc_primed && *acc_used / 16 < 0xFFFFFFFFull && !g_dbg.clear_kernel;
  if (*folded) return DTK_OK;
  if (dtk_launch_clear2(b->d_acc, *acc_used, b->d_bits, fold ? 0 : (size_t)EVB_KINDS * b->bit_words * 4, b->stream))
    return hip_fail(hipGetLastError(), "clear");
  b->acc_primed = true;
  return DTK_OK;
}

// The first pass in one of three shapes, chosen here and nowhere else (one lane per document, split, fused), then,
// chunked, the fix launch unless the scan carries its step (*fix_in_scan), and the device-side rounds.  Marks 3..7 end
// start records, link, walk, verify, fix: an interval without a launch stays empty, the rounds fall into the scan's.
static int first_pass(const dtk_model *m, dtk_batch *b, const DtkSpecArgs &sp, bool *fix_in_scan) {
  int rc;
  if (b->has_carry)
    HIP_TRY(hipMemcpyAsync(b->d_init_rec, b->h_init_rec.p, sizeof(DtkLaneState), hipMemcpyHostToDevice, b->stream));
  const DtkWalkArgs w = walk_args(b);
  *fix_in_scan = false;
  if (b->chunk == 0) {
    if ((rc = mark(b, 3)) || (rc = mark(b, 4))) return rc;
    if (dtk_launch_walk(&m->tab, &w, b->stream)) return hip_fail(hipGetLastError(), "walk");
    if ((rc = mark(b, 5)) || (rc = mark(b, 6))) return rc;
    return mark(b, 7);
  }
  uint32_t *nb = b->d_totals->n_bad;  // nb[0]: broken documents after the first pass, nb[r + 1]: after round r
  auto spec = [&](DtkSpecStage stage) { return launch_spec(b, &w, &sp, stage, nb, "speculative walk"); };
  // DATOK_SPLIT_START=1: start records and chunk walk as two launches (the repair rounds' kernels)
  const bool split = g_dbg.split_start != 0 || sp.lds_words == 0;  // (k_spec_both reports through the wave's LDS bitmaps)
  // Device-side repair: if the batch's last run had to repair (text with tags, say), two repair rounds are
  // enqueued right behind the first pass; their kernels return at once when the verification before them found
  // nothing broken, and the scan / compaction behind them only run once nothing is.  A miss then costs no host
  // round trip.  (Not done blindly: ten empty launches cost a clean corpus some 15 us per batch.)
  b->dev_rounds = g_dbg.dev_rounds >= 0 ? (uint32_t)g_dbg.dev_rounds : (b->expect_repairs ? 2u : 0u);
  if (b->dev_rounds > 3u) b->dev_rounds = 3u;
  // k_spec_fix's step rides in the one-launch scan (not for a slice of a stream: k_stream_cut, in front of the scan,
  // has to know whether the document is broken)
  *fix_in_scan = b->n_docs <= DTK_SCAN_TILES_MAX_DOCS && b->dev_rounds == 0 && !is_slice(b);
  if (split) {
    if ((rc = spec(DTK_SPEC_START)) || (rc = mark(b, 3)) || (rc = spec(DTK_SPEC_LINK)) || (rc = mark(b, 4)) ||
        (rc = spec(DTK_SPEC_WALK)) || (rc = mark(b, 5)) || (rc = spec(DTK_SPEC_VERIFY)) || (rc = mark(b, 6)))
      return rc;
  } else {  // (start records + walk are timed as "walk")
    if ((rc = mark(b, 3)) || (rc = mark(b, 4)) || (rc = spec(DTK_SPEC_START_WALK)) || (rc = mark(b, 5)) ||
        (rc = spec(DTK_SPEC_LINK_VERIFY)) || (rc = mark(b, 6)))
      return rc;
  }
  if ((!*fix_in_scan && (rc = spec(DTK_SPEC_FIX))) || (rc = mark(b, 7))) return rc;
  for (uint32_t r = 0; r < b->dev_rounds; r++)
    if ((rc = repair_round(b, &w, nb + r, nb + r + 1)) != DTK_OK) return rc;
  return DTK_OK;
}

// The tail of a run: the slice's cut, the row offsets from the walk's own counts (no counting pass), the rows, the
// totals.  in_run, from dtk_batch_run: every kernel looks at the run's count of broken documents first (chunked), the
// scan does k_spec_fix's step if fix_spec is set, k_to_host copies.  Else from finish(), behind the host's rounds.
static int run_tail(dtk_batch *b, bool in_run, const DtkSpecArgs *fix_spec, DtkCompactWhich which) {
  uint32_t *skip_if = in_run && b->chunk ? b->d_totals->n_bad + b->dev_rounds : nullptr;
  int rc;
  if (is_slice(b) && (rc = launch_stream_cut(b, skip_if)) != DTK_OK) return rc;
  if (dtk_launch_scan3(b->d_tok_cnt, b->d_sent_cnt, b->d_text_cnt, b->d_tok_off, b->d_sent_off, b->d_text_off, b->n_docs,
                       &b->d_totals->n_tok, b->d_status, b->d_scan_ws, fix_spec, in_run ? b->d_redo.p : nullptr,
                       in_run ? b->d_totals->n_bad : nullptr, skip_if, b->stream))
    return hip_fail(hipGetLastError(), "scan");
  if (in_run && (rc = mark(b, 8)) != DTK_OK) return rc;
  if ((rc = launch_compact(b, which, skip_if)) != DTK_OK) return rc;
  if (in_run) {
    if ((rc = mark(b, 9)) != DTK_OK) return rc;
    b->eager_fields = 0; b->results_changed = false;
    if ((b->fields & DTK_R_EAGER) && (rc = launch_to_host(b)) != DTK_OK) return rc;
  }
  HIP_TRY(hipMemcpyAsync(b->h_totals, b->d_totals, DTK_TOTALS_BYTES, hipMemcpyDeviceToHost, b->stream));
  return DTK_OK;
}

extern "C" int dtk_batch_run(const dtk_model *m, dtk_batch *b, uint32_t flags) {
  if (!m || !b) return DTK_E_ARG;
  if (b->n_docs == 0 || !b->d_off) return DTK_E_STATE;
  if (m->device != b->device) return DTK_E_ARG;
  // a slice of a stream is one document, and an open end has bytes behind it
  if (is_slice(b) && (b->n_docs != 1 || b->total <= b->open_slice)) return DTK_E_ARG;
  int rc;
  if ((rc = plan_lanes(b)) != DTK_OK || (rc = settle_last_run(b)) != DTK_OK) return rc;
  b->last_model = m; b->last_flags = flags; b->repair_rounds = 0;
  size_t acc_used = 0;
  bool acc_folded = false, fix_in_scan = false;
  if ((rc = mark(b, 0)) != DTK_OK || (rc = clear_accumulators(b, &acc_used, &acc_folded)) != DTK_OK || (rc = mark(b, 1)) != DTK_OK)
    return rc;
  if (dtk_launch_symbolize(b->d_text, b->d_off, b->n_docs, b->total, &m->sig, b->d_sym,
                           b->d_text == b->d_text_own, b->d_blk_doc, (unsigned long long *)&b->d_totals->invalid_epoch,
                           (uint32_t *)b->d_rsbits.p, b->d_bits, b->bit_words, acc_folded ? b->d_acc.p : nullptr, acc_used,
                           ++b->epoch, b->stream))
    return hip_fail(hipGetLastError(), "symbolize");
  const DtkSpecArgs sp = spec_args(b, false);
  if ((rc = mark(b, 2)) != DTK_OK || (rc = first_pass(m, b, sp, &fix_in_scan)) != DTK_OK) return rc;
  // (the kernel for documents with EOT calls only if this batch object's last run had such documents, or with every run
  //  for the tests; finish() launches it when the other kernel reports one after all)
  b->ran_full = false;
  const bool both = b->expect_eot || g_dbg.compact_full != 0;
  if ((rc = run_tail(b, true, fix_in_scan ? &sp : nullptr, both ? DTK_COMPACT_BOTH : DTK_COMPACT_PLAIN)) != DTK_OK) return rc;
  if ((rc = b->ev_ran.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev_ran, b->stream));
  b->ev_ran_valid = true; b->ran = true; b->totals_valid = false; b->render_flags = 0xFFFFFFFFu;
  return DTK_OK;
}

// 1: everything dtk_batch_run enqueued has finished (dtk_batch_totals & co. will not wait for the GPU unless the
// run needs a repair); 0: not yet; never blocks.  (An event query: hipStreamQuery on a busy stream was seen to
// return only when the stream had drained.)
extern "C" int dtk_batch_done(dtk_batch *b) {
  if (!b || !b->ran || !b->ev_ran) return 0;
  const hipError_t e = hipEventQuery(b->ev_ran);
  if (e != hipSuccess) (void)hipGetLastError();
  return e == hipSuccess ? 1 : 0;
}

// The exact pass (k_exact_doc): documents flagged ST_IRREGULAR by the walk are walked again by one lane each,
// which writes their rows of the result arrays in the reference's call order and lists their calls.  Rare
// by construction (no shipped model produces one on any test corpus), hence the host round trips.
static int run_exact(dtk_batch *b) {
  const dtk_model *m = b->last_model;
  hipStream_t s = b->stream;
  const uint32_t nd = b->n_docs;
  std::vector<uint32_t> st(nd);
  HIP_TRY(hipMemcpy(st.data(), b->d_status, (size_t)nd * 4, hipMemcpyDeviceToHost));
  for (uint32_t d = 0; d < nd; d++)
    if (st[d] & ST_IRREGULAR) b->h_exact_ids.push_back(d);
  const uint32_t n = (uint32_t)b->h_exact_ids.size();
  if (n == 0) return DTK_OK;
  if (n > b->exact_cap) {
    const uint64_t cap = (uint64_t)n + n / 4 + 16;
    int rc;
    b->exact_cap = 0;
    if ((rc = b->d_exact_ids.fit(cap, cap)) || (rc = b->d_exact_cnt.fit(cap, cap)) || (rc = b->d_exact_off.fit(cap + 1, cap + 1)))
      return rc;
    b->exact_cap = (uint32_t)cap;
  }
  HIP_TRY(hipMemcpy(b->d_exact_ids, b->h_exact_ids.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  DtkExactArgs X{};
  X.sym = sym_of(b); X.text = b->d_text; X.doc_off = b->d_off; X.n = n; X.docs = b->d_exact_ids;
  X.n_calls = b->d_exact_cnt; X.call_off = b->d_exact_off; X.status = b->d_status;
  X.flags = b->last_flags & DTK_NEWLINE_AFTER_EOT; X.step_factor = walk_args(b).step_factor;
  set_outputs(b, X);
  X.pass = 0;
  if (dtk_launch_exact(&m->tab, &X, s)) return hip_fail(hipGetLastError(), "exact pass (count)");
  std::vector<uint32_t> cnt(n);
  HIP_TRY(hipMemcpyAsync(cnt.data(), b->d_exact_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  b->h_exact_off.assign((size_t)n + 1, 0);
  for (uint32_t i = 0; i < n; i++) b->h_exact_off[i + 1] = b->h_exact_off[i] + cnt[i];
  const uint64_t total = b->h_exact_off[n];
  if (const int rc = b->d_calls.fit(total, total + total / 4 + 16)) return rc;
  HIP_TRY(hipMemcpy(b->d_exact_off, b->h_exact_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
  X.calls = b->d_calls;
  X.pass = 1;
  if (dtk_launch_exact(&m->tab, &X, s)) return hip_fail(hipGetLastError(), "exact pass");
  b->h_calls.resize((size_t)total);
  if (total) HIP_TRY(hipMemcpyAsync(b->h_calls.data(), b->d_calls, (size_t)total * sizeof(DtkCall), hipMemcpyDeviceToHost, s));
  // the documents' status words were rewritten: count the flagged ones again
  HIP_TRY(hipMemcpyAsync(st.data(), b->d_status, (size_t)nd * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  uint64_t flagged = 0;
  for (uint32_t d = 0; d < nd; d++) flagged += st[d] != 0;
  b->h_totals->n_flagged = flagged;
  return DTK_OK;
}

// DtkDebug::debug_repair: the lane records of the first three documents that a round left broken
static int dump_broken(dtk_batch *b, uint32_t left) {
  std::vector<uint32_t> redo(b->n_docs), chunk_off(b->n_docs + 1);
  HIP_TRY(hipMemcpy(redo.data(), b->d_redo, (size_t)b->n_docs * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(chunk_off.data(), b->d_chunk_off, ((size_t)b->n_docs + 1) * 4, hipMemcpyDeviceToHost));
  for (uint32_t d = 0, shown = 0; d < b->n_docs && shown < 3; d++)
    if (redo[d] != 0xFFFFFFFFu) {
      const uint32_t L0 = chunk_off[d], L1 = chunk_off[d + 1], n = std::min<uint32_t>(L1 - L0, 24u);
      std::vector<DtkLaneState> st(n), en(n);
      HIP_TRY(hipMemcpy(st.data(), b->d_lane_start + L0, n * sizeof(DtkLaneState), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(en.data(), b->d_lane_end + L0, n * sizeof(DtkLaneState), hipMemcpyDeviceToHost));
      fprintf(stderr, "round %u: %u broken; doc %u lanes %u redo from lane %u:", b->repair_rounds, left, d, L1 - L0, redo[d] - L0);
      for (uint32_t k = 0; k < n; k++)
        fprintf(stderr, " [%u: s %d/%u/%x e %d/%u/%x]", k, (int)st[k].p, st[k].t, st[k].flags, (int)en[k].p, en[k].t, en[k].flags);
      fprintf(stderr, "\n");
      shown++;
    }
  return DTK_OK;
}

// Speculation check failed somewhere: those documents are repaired from the last owning lane before their first
// bad lane on (fix records, clear, re-link, re-walk, re-verify) until every lane chains.  Rounds enqueued ahead of
// time (dtk_batch_run) have run on the device already; what is still broken behind them is repaired from here,
// and the tail -- which did nothing in that case -- runs afterwards.  *finished: the fallback has finished the run.
static int repair_from_host(dtk_batch *b, bool *finished) {
  const uint32_t *hnb = b->h_totals->n_bad;
  for (uint32_t r = 0; r < b->dev_rounds; r++)
    if (hnb[r] != 0) b->repair_rounds++;
  uint32_t left = hnb[b->dev_rounds];
  if (left != 0) {
    b->results_changed = true;
    hipStream_t s = b->stream;
    DtkWalkArgs w = walk_args(b);
    uint32_t *n_bad = b->d_totals->n_bad + b->dev_rounds;  // (the counter the scan / compaction looked at)
    // Every round verifies at least one more lane of every broken document (the first bad lane started from a true
    // state), so the longest document's lane count bounds the rounds.  Should they run out all the same, the batch
    // is walked again with one lane per document -- no speculation, nothing to repair.
    const uint32_t max_rounds = b->max_doc_lanes + 16u;
    int rc;
    while (left != 0) {
      b->repair_rounds++;
      HIP_TRY(hipMemsetAsync(n_bad, 0, 4, s));
      if ((rc = repair_round(b, &w, nullptr, n_bad)) != DTK_OK) return rc;
      HIP_TRY(hipMemcpyAsync(&left, n_bad, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (left != 0 && g_dbg.debug_repair && b->repair_rounds < 12 && (rc = dump_broken(b, left)) != DTK_OK) return rc;
      if (left != 0 && (b->repair_rounds > max_rounds || b->repair_rounds >= b->round_limit)) {
        const uint32_t rounds = b->repair_rounds, keep = b->cfg_chunk;
        b->cfg_chunk = 0; b->plan_valid = false;
        rc = dtk_batch_run(b->last_model, b, b->last_flags);
        if (rc == DTK_OK) rc = finish(b);
        b->cfg_chunk = keep; b->plan_valid = false;
        b->repair_rounds = rounds; b->totals.repair_rounds = rounds;
        b->expect_repairs = true;
        *finished = true;
        return rc;
      }
    }
    if ((rc = run_tail(b, false, nullptr, DTK_COMPACT_BOTH)) != DTK_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s));
  }
  b->expect_repairs = b->repair_rounds != 0;
  return DTK_OK;
}

// Arrays the compaction found too small grow (the only allocation that can follow a run) and both kernels run again;
// then the EOT kernel, if there are such documents and it has not run.  any_irregular and any_eot (one word) are read again.
static int compact_again(dtk_batch *b) {
  auto again = [b](DtkCompactWhich which) -> int {
    b->results_changed = true;
    if (const int rc = launch_compact(b, which, b->last_args.skip_if)) return rc;
    HIP_TRY(hipMemcpyAsync(&b->h_totals->any_irregular, &b->d_totals->any_irregular, 8, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return DTK_OK;
  };
  const uint64_t nt = b->h_totals->n_tok, ns = b->h_totals->n_sent, nx = b->h_totals->n_text;
  int rc;
  if (nt > b->tok_cap || ns > b->sent_cap || nx > b->text_cap) {
    b->results_changed = true;
    if ((rc = alloc_outputs(b, nt + nt / 8 + 16, ns + ns / 8 + 16, nx + nx / 8 + 16)) != DTK_OK) return rc;
    if ((rc = again(DTK_COMPACT_BOTH)) != DTK_OK) return rc;
  }
  const bool eot = b->h_totals->any_eot != 0;
  if (eot && !b->ran_full && (rc = again(DTK_COMPACT_EOT)) != DTK_OK) return rc;
  b->expect_eot = eot;
  return DTK_OK;
}

// Completes the last run: reads its totals and does what they ask for.
int finish(dtk_batch *b) {
  if (!b->ran) return DTK_E_STATE;
  if (b->totals_valid) return DTK_OK;
  int rc;
  if ((rc = wait_own(b)) != DTK_OK) return rc;  // (on a lent stream: this batch's run, not its neighbours')
  bool finished = false;
  if (b->chunk != 0 && ((rc = repair_from_host(b, &finished)) != DTK_OK || finished)) return rc;
  DtkTotalsDev *h = b->h_totals;
  b->n_invalid = h->invalid_epoch == b->epoch ? 1u : 0u;  // (the number of the last run that saw one: k_symbolize)
  if ((rc = compact_again(b)) != DTK_OK) return rc;
  // documents whose calls are not in position order (ST_IRREGULAR): their rows come from the exact pass
  b->h_exact_ids.clear(); b->h_exact_off.assign(1, 0); b->h_calls.clear();
  if (h->any_irregular != 0) {
    // (the exact pass walks a document from its beginning in a new writer's terms: not from a carried record, and
    //  not up to a cut)
    if (is_slice(b)) return DTK_E_IRREGULAR;
    b->results_changed = true;
    if ((rc = run_exact(b)) != DTK_OK) return rc;
  }
  // the arrays k_to_host brought over inside the run count if the kernel made its copy and nothing was touched since
  if (b->eager_fields && !b->results_changed && h->to_host_epoch == b->epoch) {
    b->dl_begun = b->dl_waited = true; b->dl_fields = b->eager_fields;
  }
  dtk_totals &t = b->totals;
  t.n_docs = b->n_docs; t.n_bytes = b->total; t.walk_steps = 0;
  t.n_tokens = h->n_tok; t.n_sent = h->n_sent; t.n_texts = h->n_text; t.n_flagged = h->n_flagged;
  for (uint32_t i = 0; i < DTK_STEP_STRIPES; i++) t.walk_steps += *dtk_step_stripe(h, i);
  t.n_lanes = b->chunk ? b->n_lanes : b->n_docs; t.chunk_bytes = b->chunk; t.repair_rounds = b->repair_rounds;
  b->totals_valid = true;
  return DTK_OK;
}
