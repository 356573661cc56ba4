// dtk_host.h -- what the host units of libdatok_gpu.so (dtk_model, dtk_foma, dtk_batch, dtk_run, dtk_results, dtk_derived, dtk_slice .cpp) share:
// the model and batch objects, the error state, the test hooks, and helpers (hidden, not exported).  No .hip unit includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/datok_gpu.h"
#include "dtk_internal.h"
#include "dtk_own.h"  // the error state (hip_fail, HIP_TRY) and the owning types
#include "dtk_mirror.h"
#include "dtk_vocab_core.h"
#include "dtk_wordpiece_core.h"
#include "dtk_encode_core.h"

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------- test hooks
//
// The library's behaviour does not depend on the caller's environment: nothing here reads it.  The switches
// below select code paths that the library otherwise picks by model, shape or history, so that the tests can run the
// whole suite over each of them; only dtk_debug_configure sets them (the Python harness forwards DATOK_* variables
// to it, datok_amd/_lib.py -- the shipped entry points never look).  None of them changes a result.
struct DtkDebug {
  int sym16 = 0;         // 16-bit stream entries although the model's entries fit a code table
  int general16 = 0;     // a stream of 16-bit entries is walked by the general loop (as before the lean loop read them): A/B timing
  int force_wide = 0;    // 32-bit plain cells for any model (MatrixTrans<uint32_t>)
  int file_columns = 0;  // keep the file's column order
  int no_fused = 0;      // plain cells (uint16, uint32 from 32 767 states on): no fused epsilon + rune cells
  int wide_fused = 0;    // 64-bit fused cells for any model (else only where the state ids do not fit 15 bits)
  int no_dense = 0;      // walk a double array's {base, check} pairs instead of its dense layout
  int small_max = -1;    // documents of at most this many bytes are compacted one per lane (-1: by batch shape)
  int lds_bits = 1;      // 0: event bits straight to memory
  int split_start = 0;   // start records and chunk walk as two launches
  int dev_rounds = -1;   // repair rounds enqueued with every run (-1: two after a run that had to repair)
  int compact_full = 0;  // both compaction kernels with every run
  int clear_kernel = 0;  // the accumulator block is cleared by k_clear2, not by k_symbolize's blocks
  int round_limit = -1;  // host repair rounds before the one-lane-per-document fallback (-1: the longest document's lanes)
  int debug_repair = 0;  // print the lane records of documents that stay broken
  int blk_span = -1;     // what a segment of a 64-token block may span in the blocked offsets (-1 or 0: 65 535); read where
                         // k_pack_blk is launched, so that ordinary text reaches the fallback to the 32-bit arrays (and where
                         // a stream's k_so_pack64 is: the fallback to the plain 64-bit arrays)
  int evl_cap = -1;      // entries the copies of DTK_R_EVENT_LIST are first sized for, in place of n_sent + n_texts (-1: off),
                         // so that ordinary text reaches the second download of a list that outgrew the bound; a stream's offset
                         // delivery also sizes its first copies of sent and the text rows with it (the late copy at delivery)
  int sen_cap = -1;      // rows the sentence table (DTK_R_SENTENCES) is first sized for, in place of n_sent (-1: off), so that
                         // ordinary text reaches the second build of a table that outgrew the bound
  int vocab_hash_bits = -1;  // a vocabulary built from now on keeps only this many low bits of its hash, in the builder, the host
                         // probe and the kernel alike (-1: off), so that a handful of words collide, share tags and wrap
  long long sp_posc0 = 0; // posC in front of a stream's first slice in a position mode or with offset delivery (dtk_stream_run reads it once, at its
                         // start): integers beyond 2^32 and of 11 digits from a stream of a few hundred bytes
};
extern DtkDebug g_dbg;

// ------------------------------------------------------------------- model

struct dtk_model {
  int kind = 0;
  int epsilon = 0, unknown = 0, identity = 0, final_state = 0, sigma_count = 0;
  uint32_t state_count = 0;
  std::vector<uint16_t> col;   // symbol -> column of the device table (layout_matrix); empty: the symbol itself
  uint32_t dense_states = 0;   // double array laid out as a matrix (densify in build_datok): its states; 0: the pairs are walked
  uint64_t array_len = 0;
  uint32_t n_eps_states = 0, max_eps_chain = 0, unknown_used = 0;
  uint32_t lean_walk = 0;      // dtk_batch_run walks this model with the lean loop (build_images)
  uint64_t device_bytes = 0;
  int device = 0;
  bool host_only = false;      // dtk_model_info_mem: the host images are built and measured, nothing is copied to a device
  // host copy of the sigma map, for rendering (Go string(rune) of a token surface)
  std::vector<uint32_t> sigma_runes;
  std::vector<uint16_t> sigma_syms;
  uint16_t ascii[256];
  // device
  DevArray<uint8_t> d_tab;
  DevArray<uint16_t> d_ascii;
  DevArray<uint32_t> d_runes;
  DevArray<uint16_t> d_syms;
  DevArray<uint8_t> d_codes;  // code_entry [256] u16, code_lt256 [256] u8, code_runes [n_runes] u8
  DtkTableDev tab{};
  DtkSigmaDev sig{};
};

int go_decode_host(const uint8_t *p, size_t n, uint32_t *r);
int gunzip(const uint8_t *gz, size_t n, std::vector<uint8_t> &out);
bool special_ids_ok(const dtk_model *m);
int layout_matrix(dtk_model *m, const std::vector<uint32_t> &arr, uint64_t n_states, bool da_dense);
int build_foma(dtk_model *m, const std::vector<uint8_t> &raw);

// ------------------------------------------------------ vocabulary and tally (dtk_vocab.cpp)
//
// The table of dtk_vocab_core.h on one device, immutable after creation; the counters of dtk_tally beside it.
struct dtk_vocab {
  int device = 0;
  uint32_t n_words = 0;
  DevArray<uint64_t> d_slots;
  DevArray<uint32_t> d_off, d_bytes;  // (the words' bytes in whole 32-bit words: the kernel reads them as such)
  DtkVocabDev dev{};
};
// the words' longest, in bytes (DtkVocabDev::max_word)
uint32_t vocab_max_word(const uint64_t *off, uint32_t n_words);
// a split's arguments checked (DTK_E_ARG) and made into the rule of dtk_wordpiece_core.h
int wordpiece_rule(uint32_t n_words, const uint8_t *prefix, uint32_t prefix_len, int32_t unk_id, uint32_t max_runes,
                   DtkWpRule *rule);
struct dtk_tally {
  int device = 0;
  uint32_t n_words = 0;
  DevArray<unsigned long long> d_counts;  // n_words + 1, the last: unknown
};

// ------------------------------------------------------ fold (dtk_fold.cpp)
//
// The tables of dtk_fold_core.h in one array of 32-bit words: the entry blocks, the multi array, the page table.
struct FoldImage {
  std::vector<uint32_t> words;
  size_t multi_at = 0, page_at = 0;  // where the two begin, in words
  DtkFoldDev view(const uint32_t *base) const {
    return DtkFoldDev{base, reinterpret_cast<const uint16_t *>(base + page_at), base + multi_at};
  }
};
// a fold's arguments checked (DTK_E_ARG) and made into the tables
int fold_image(const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n, FoldImage &img);
// The tables on one device, immutable after creation.
struct dtk_fold {
  int device = 0;
  DevArray<uint32_t> d_words;
  DtkFoldDev dev{};
};

// ------------------------------------------------------ a stream slice's device outputs
//
// What the next download of a batch that is a slot of a stream (dtk_streamer.cpp) computes beside the result arrays, on
// the download stream behind every packing of the event list (dtk_slice.cpp).  A default-constructed request: nothing.
struct SliceRequest {
  uint32_t first = 0, cut = 0;  // the slice's calls: those of the window bytes [first, cut]
  bool last = false;            // ... and the tail word's (the stream's last slice)
  // NewTokenWriter(w, bits)'s bytes for these calls: in a position-free mode (dtk_stream_set_render,
  // dtk_streamrender.hip; bits: TOKENS | SENTENCES) or in a position mode (dtk_stream_set_position_render,
  // dtk_streampos.hip; all five writer bits)
  enum Bytes : uint8_t { kNoBytes, kPlainBytes, kPosBytes } bytes = kNoBytes;
  uint32_t bits = 0;
  // the writer's rune offsets and sentence list as arrays (dtk_stream_set_offsets, dtk_streamoffs.hip), beside the
  // position-free bytes or without them
  bool offs = false;
  uint32_t form = 0;            // DTK_SO_*
  // the sentences as rows (dtk_stream_set_sentences, dtk_streamsens.hip), behind the offsets chain, which then runs
  // whether offs is set or not (without it: in the plain form, and nothing of its arrays comes home)
  bool sens = false;
  uint64_t base = 0;            // sens: stream offset of window byte 0
  const DtkSenCarry *sen_carry_in = nullptr;  // sens: the open row comes from one of the stream's slots and goes into another
  DtkSenCarry *sen_carry_out = nullptr;
  bool is_matrix = false;
  bool nl = false;              // the run's NEWLINE_AFTER_EOT (offsets; a position mode has it in bits)
  uint32_t digits = 0;          // kPosBytes: no integer of the slice has more bytes (the stream's bound)
  // kPosBytes, offs or sens: the writer's state comes from one of the stream's carry slots and goes into another
  const DtkPosCarry *carry_in = nullptr;
  DtkPosCarry *carry_out = nullptr;
};
// What comes home lies in blocks of dtk_mirror.h, described anew for every slice (dtk_slice.cpp): each piece below is
// both a device array the kernels write and its page-locked copy.  The first copies bring a piece as far as the
// compaction's counts reach, and the trailer; what the trailer then asks for beyond that (blk_fail: the plain offsets;
// more sent ints or rows) is copied at delivery -- the pieces' home counts say what is there.
struct SliceOut {
  SliceRequest req;
  DevArray<uint64_t> d_ws, d_offs_ws, d_sens_ws;  // the units' workspaces (tile sums and scans)
  struct Bytes : MirrorBlock {  // the rendering under way: the bytes, then the length word (kPlainBytes) or the trailer (kPosBytes)
    Piece<uint8_t> out;
    Piece<uint64_t> len;
    Piece<DtkPosTrailer> trailer;
  } bytes;
  struct Offs : MirrorBlock {
    Piece<int64_t> rstart, rend, sent;  // tokens (exact), tokens, sent ints
    Piece<DtkOffsTrailer> trailer;
    Piece<uint32_t> ttok, tsent;        // texts
    Piece<DtkOffBlock64> heads;         // the blocked form, else empty
    Piece<uint32_t> words;
    bool blocked = false;
  } offs;
  struct Sens : MirrorBlock {
    Piece<DtkSensTrailer> trailer;
    Piece<uint32_t> tse, tok_end;       // texts, rows
    Piece<uint64_t> bstart, bend;       // rows
    Piece<int64_t> rstart, rend;
    uint64_t n = 0;                     // the slice's tokens
  } sens;
};

// -------------------------------------------------------------------- batch

struct dtk_batch {
  ~dtk_batch();  // waits for what is in flight; the members then release themselves, in reverse order
  int device = 0;
  Stream stream;  // (declared before the memory: destroyed after it)
  uint64_t max_bytes = 0;
  uint32_t max_docs = 0;
  // inputs
  DevArray<uint8_t> d_text_own;
  DevArray<uint64_t> d_off_own;
  const uint8_t *d_text = nullptr;
  const uint64_t *d_off = nullptr;
  uint32_t n_docs = 0;
  uint64_t total = 0;
  // intermediates
  DevArray<uint16_t> d_sym;
  DevArray<uint8_t> d_rsbits;                  // rune-start bitmap of the input (1 bit per byte, read as 32-bit words)
  DevArray<uint32_t> d_bits;                   // event bitmaps of the walk (EVB_KINDS kinds), cleared every run
  uint32_t bit_words = 0;                      // words per kind of the current input
  uint32_t *d_doc_tail = nullptr;              // per document: final SentenceEnd / TextEnd (carved from d_acc)
  DevArray<uint8_t> d_acc;                     // per-document accumulators + totals (one memset)
  uint32_t *d_status = nullptr;
  // speculative chunk lanes
  std::vector<uint64_t> h_doc_off;   // host copy of the document offsets (lane planning)
  uint32_t cfg_chunk = 0xFFFFFFFFu;  // 0 = one lane per document, 0xFFFFFFFF = automatic
  uint32_t cfg_extend = 240;         // move the warm-up start back to the previous blank, at most this far
  uint32_t cfg_warm = 8;             // (16 until round 3: 8 costs no repair round on any corpus and 5 % fewer lookups) plus the way back to the previous blank (cfg_extend); a miss only costs a repair round
  uint32_t chunk = 0;                // chunk size of the current plan (0 = none)
  bool plan_valid = false;
  uint32_t n_lanes = 0, lane_cap = 0;
  DevArray<uint32_t> d_lane_doc, d_chunk_off, d_redo;
  // long documents are compacted in segments of DTK_SEG_LANES lanes (tables built with the lane plan)
  DevArray<uint32_t> d_seg_tab;      // seg_doc | seg_lane0 | seg_nl | doc_seg0
  DevArray<DtkSegSum> d_seg_sum;
  DevArray<DtkSegIn> d_seg_in;
  uint32_t n_segs = 0, seg_cap = 0;
  bool long_docs = false;            // some document has more than one segment
  uint32_t max_doc_lanes = 0;        // lanes of the longest document (bounds the repair rounds)
  DevArray<uint32_t> d_blk_doc;      // document of the first byte of every 4 KiB input block
  // compaction: documents of at most small_max bytes go one per lane (k_compact_small), the others one per wave
  uint32_t small_max = 0, n_big = 0;
  DevArray<uint32_t> d_big_docs;     // ids of the documents above small_max
  uint32_t *d_first_bad = nullptr, *d_fail_lane = nullptr;  // (carved from d_acc)
  DevArray<DtkLaneCount> d_lane_cnt;
  DevArray<DtkLaneState> d_lane_start, d_lane_end;
  DevArray<DtkLanePlan> d_lane_plan;
  uint32_t repair_rounds = 0;        // of the last run
  const dtk_model *last_model = nullptr;
  uint32_t last_flags = 0;
  DevArray<uint64_t> d_csr;  // tok_off | sent_off | text_off
  uint64_t *d_tok_off = nullptr, *d_sent_off = nullptr, *d_text_off = nullptr;
  uint64_t *d_tok_cnt = nullptr, *d_sent_cnt = nullptr, *d_text_cnt = nullptr;  // per-document counts
  DevArray<uint64_t> d_scan_ws;  // tile sums of the multi-block scan (many documents)
  DtkTotalsDev *d_totals = nullptr;  // the head of d_acc
  uint32_t dev_rounds = 0;       // repair rounds enqueued ahead of time in the last run
  bool expect_repairs = false;   // the last run needed repairs: enqueue rounds ahead of time in the next one
  uint32_t round_limit = 0xFFFFFFFFu;  // repair rounds from the host before the one-lane-per-document fallback (DATOK_ROUND_LIMIT)
  bool acc_primed = false;       // the accumulator block has been cleared whole once (k_symbolize clears it from then on)
  uint64_t epoch = 0;            // number of the run (k_symbolize marks runs that saw invalid UTF-8 with it)
  bool expect_eot = false;       // the last run had documents with EOT calls: launch their compaction kernel with the run
  bool ran_full = false;         // that kernel has run since the last dtk_batch_run
  PinBuf h_totals_pin;           // d_totals and the lookup counters behind it (DTK_TOTALS_BYTES), as the run left them
  DtkTotalsDev *h_totals = nullptr;
  PinBuf h_off_pin;              // staging of the document offsets (a copy from pageable memory would block until
                                 // the text copy in front of it has finished: 0.7 ms per 16 MiB batch)
  // outputs (grown on demand, never inside a run unless a re-launch is needed)
  uint64_t tok_cap = 0, sent_cap = 0, text_cap = 0;
  DevArray<int32_t> d_rstart, d_rend, d_sent;
  DevArray<uint32_t> d_bstart, d_bend, d_ttok, d_tsent;
  DevArray<uint32_t> d_sbefore, d_ts_end, d_doc_ns;  // renderer inputs (compact)
  // device rendering of the writer output (dtk_batch_render): workspace + output, grown on demand
  DevArray<uint64_t> d_rws;   // scans, tile sums, per-text regions (u64 words)
  DevArray<uint64_t> d_out_off;
  DevArray<uint8_t> d_out;
  uint64_t out_total = 0;
  uint64_t n_invalid = 0;     // nonzero: the last run saw invalid UTF-8 (each such byte prints as U+FFFD, 3 bytes)
  uint32_t render_flags = 0xFFFFFFFFu;  // flags of the rendering held in d_out (none)
  std::vector<uint8_t> h_out;
  std::vector<uint64_t> h_out_off;
  // the exact pass over ST_IRREGULAR documents (normally none): ids, call counts / offsets, calls
  DevArray<uint32_t> d_exact_ids, d_exact_cnt;
  DevArray<uint64_t> d_exact_off;
  DevArray<DtkCall> d_calls;
  uint32_t exact_cap = 0;
  std::vector<uint32_t> h_exact_ids;
  std::vector<uint64_t> h_exact_off;
  std::vector<DtkCall> h_calls;
  // optional stage timing
  bool profiling = false;
  Event ev[DTK_N_STAGES + 1];
  // last run
  bool ran = false, totals_valid = false;
  DtkCompactArgs last_args{};
  dtk_totals totals{};
  // Results on the host (dtk_batch_result_host): page-locked buffers owned by the batch, filled by one chain of
  // asynchronous copies on a stream of their own (dl_stream) -- the batch's own stream is free for the next kernels,
  // the copy engine for the next slice's upload (PCIe is full duplex).  `fields` (DTK_R_*) selects what is copied.
  // (one buffer per row of host_arrays, dtk_results.cpp)
  enum { PB_R16, PB_RBLK, PB_RBLK_HEAD, PB_BBLK, PB_BBLK_HEAD, PB_RSTART, PB_REND, PB_BSTART, PB_BEND, PB_BITS, PB_EVL_POS, PB_EVL_KIND, PB_EVL_OFF, PB_TAIL, PB_SENT, PB_TTOK, PB_TSENT, PB_CSR, PB_STATUS,
         PB_N };
  PinBuf pin[PB_N];
  PinBuf h_plan;            // staging of the lane plan's tables (plan_lanes)
  uint32_t fields = DTK_R_ALL;
  DevArray<uint32_t> d_r16;       // DTK_R_TOK_RUNE16: the packed rune offsets (filled on the download stream)
  // DTK_R_TOK_RUNE_BLK ([0]) / DTK_R_TOK_BYTE_BLK ([1]): the blocked offsets, sized from tok_cap and packed on the
  // download stream like d_r16.  A block that does not fit 16 bits raises the pair's flag word; dtk_batch_result_host
  // reads its page-locked copy behind the download and brings the pair's 32-bit arrays in its place.
  struct BlkPair { DevArray<uint32_t> d_words; DevArray<dtk_off_block> d_heads; uint64_t cap = 0; } blk[2];  // cap: tokens
  DevArray<uint32_t> d_blk_flag;   // [2]
  PinBuf h_blk_flag;               // [2]
  uint32_t blk_pending = 0;        // blocked fields on their way whose flag nobody has looked at yet
  uint32_t blk_failed = 0;         // blocked fields the last run's offsets do not fit: the 32-bit arrays stand in
  // DTK_R_EVENT_LIST: the set bits of SEPS | TEOT | SEOT as rows, compacted on the download stream (dtk_evlist.hip).  The
  // copies are sized for n_sent + n_texts rows; the count word travels behind them, and dtk_batch_result_host copies
  // again (evl_need rows) if the list turned out longer.
  DevArray<uint32_t> d_evl_pos, d_evl_bit, d_evl_off, d_evl_tiles, d_evl_cnt;  // (d_evl_bit: device only; d_evl_cnt: [1])
  DevArray<uint8_t> d_evl_kind;
  PinBuf h_evl_cnt;                // [1]
  uint64_t evl_copied = 0;         // rows the last enqueued copies of the list hold
  uint64_t evl_need = 0;           // nonzero: this run's list has that many rows, more than the bound (dtk_batch_result_host saw it)
  bool evl_pending = false;        // a list is on its way whose count nobody has looked at yet
  // The derived tables (dtk_derived.cpp): four blocks of dtk_mirror.h, each computed on the download stream behind
  // finish() and kept by the one protocol of DerivedBlock.
  // DTK_R_SENTENCES / dtk_batch_sentences_*: the sentence table (dtk_sentences.hip) -- one copy brings all of it.  Sized
  // for n_sent rows; the count word says whether that was enough (need), as with the event list.
  struct Sen : DerivedBlock {
    Piece<uint64_t> off;                   // documents + 1
    Piece<uint32_t> tok_end, bstart, bend; // rows
    Piece<int32_t> rstart, rend;
    Piece<uint32_t> tse, cnt;              // texts; the count word
    bool done = false;                     // the count has been looked at and fits (and exact documents are spliced in)
    uint64_t n = 0;                        // rows of the finished table
  } sen;
  DevArray<uint32_t> d_sen_ws;     // device only: a row's bit | document | first token, and the tiles' two words
  // dtk_batch_set_vocab: every token of a run looked up in a vocabulary (dtk_tokenid.hip).  The unknown counter, then one
  // id per token; the counter always comes home, the ids with ids_home or when dtk_batch_token_ids_host asks.  The
  // kernel runs once per run, so a tally gets a run's tokens once however often the ids are asked for or copied.
  const dtk_vocab *vocab = nullptr;
  dtk_tally *tally = nullptr;
  bool ids_home = false;
  struct Ids : DerivedBlock {
    Piece<uint64_t> cnt;
    Piece<int32_t> id;
  } ids;
  // dtk_batch_set_wordpiece: every token of a run split into WordPiece ids (dtk_wordpiece.hip), once per run.  The two
  // counters (pieces, unknown tokens), piece_off, then the pieces' ids and ends at a capacity the host states before the
  // count is known (wp_cap_of); the counters always come home, and a run with more pieces than that is split again into
  // a block that holds them (wp_finish).  need is the most pieces a run of this batch had beyond what its first block
  // held, and is kept for the next runs.
  const dtk_vocab *wp_vocab = nullptr;
  // dtk_batch_set_fold: the fold both of them read their keys through, or null
  const dtk_fold *fold = nullptr;
  DtkWpRule wp_rule{};
  bool wp_home = false;
  struct Pieces : DerivedBlock {
    Piece<uint64_t> cnt;           // [n_pieces, n_unknown]
    Piece<uint64_t> off;           // n_tok + 1
    Piece<int32_t> id;             // the block's capacity in pieces
    Piece<uint32_t> bend;          // the same
  } pieces;
  DevArray<uint64_t> d_wp_ws;      // the scan's tile sums (tiles + 1), then 8 bytes per token between the two passes
  // dtk_batch_set_encode: the run's sentences or documents as model input rows (dtk_encode.hip), behind the split and,
  // for the sentence unit, behind the sentence table.  Sized by a bound the host states before any count is known
  // (enc_enqueue).  A run whose pieces or sentence table were made anew since (read), or whose rows outgrew the block,
  // wrote no row and is encoded again (enc_finish).
  bool enc_on = false;
  DtkEncRule enc_rule{};
  bool enc_home = false;
  struct Enc : DerivedBlock {
    Piece<int32_t> ids, word;      // rows * max_len each (word: 0 without DTK_ENC_WORD_IDS); 16-byte aligned
    Piece<uint64_t> piece0;        // rows
    Piece<uint64_t> off;           // units_cap + 1
    Piece<uint32_t> len;           // rows: the block's capacity
    DerivedReads read;             // of the enqueued encode: pieces.gen, and sen.gen (sentence unit, else 0)
  } enc;
  // [n_rows, n_cut, n_units, ok], beside the block and no piece of it: the counters always come home, and a block whose
  // rows stay on the device has no page-locked copy (fit(false)) for them to land in
  DevArray<uint64_t> d_enc_cnt;
  PinBuf h_enc_cnt;
  DevArray<uint64_t> d_enc_ws;     // the scan's tile sums (tiles + 1), then a DtkEncUnit per unit
  uint64_t max_doc_bytes = 0;     // of the current input (what decides whether the narrow form exists)
  bool max_doc_valid = false;
  Stream dl_stream;                 // created with the first download, unless the caller lends one (a pipeline's slices share one:
                                    //  the runtime maps streams onto four hardware queues, and streams that share a queue serialise)
  Event ev_ran;                     // behind the last launch of dtk_batch_run (dtk_batch_done)
  bool ev_ran_valid = false;
  // Lent streams (dtk_batch_set_streams): the batches of a pipeline share one stream for their kernels and one for their
  // uploads -- the runtime has four hardware queues, and a pipeline of any depth then needs three (kernels, uploads,
  // downloads).  The upload's end is an event the kernels wait for.
  hipStream_t up_stream = nullptr;  // null: uploads run on `stream`
  Event ev_up;
  bool up_pending = false;          // an upload on up_stream has not been waited for yet
  // A slice of one long stream (dtk_streamer.cpp, batch_set_slice): the batch's one document is a window of the stream.
  // open_slice != 0: the window's end is not the stream's -- k_stream_cut ends the document at the first sync point at
  // or behind that many bytes; has_carry: the walk starts from the record in h_init_rec (the previous slice's cut).
  uint32_t open_slice = 0;
  bool has_carry = false;
  DevArray<DtkLaneState> d_init_rec, d_open_fin;  // [1] each
  PinBuf h_init_rec;
  SliceOut slice;  // what the slice brings home beside the result arrays (dtk_slice.cpp)
  uint32_t eager_fields = 0;  // the last run's k_to_host was asked for these (0: none); finish() decides whether it counts
  bool results_changed = false;  // finish() had to touch the result arrays after the run (repair, growth, EOT kernel, exact pass)
  Event ev_dl;                 // behind the batch's copies on the (possibly shared) download stream
  bool dl_waited = true;
  bool dl_begun = false;    // the copies of the last run's results have been enqueued
  uint32_t dl_fields = 0;   // ... these fields
};

int wait_own(dtk_batch *b);
int wait_ran(dtk_batch *b);  // (dtk_batch.cpp, as alloc_outputs: what dtk_run.cpp needs of the object)
int alloc_outputs(dtk_batch *b, uint64_t tok, uint64_t sent, uint64_t text);
DtkSym sym_of(const dtk_batch *b);
DtkWalkArgs walk_args(dtk_batch *b);
int finish(dtk_batch *b);
int launch_to_host(dtk_batch *b);
// dtk_derived.cpp: what the four derived tables last enqueued has finished -- the input, the result arrays and the tables'
// blocks may be touched again.  Every stage is waited for even after a failure; the first failure is returned.
int derived_wait(dtk_batch *b);
// ... and what the next download enqueues of them, each in its own state (dtk_batch_download_begin)
int derived_enqueue(dtk_batch *b);
int sen_enqueue(dtk_batch *b, bool home);  // DTK_R_SENTENCES: the table's kernels and the copy of its block
bool enc_rule_of(const dtk_encode_spec *s, DtkEncRule *r);  // dtk_encode.cpp: a spec checked and made into the rule (false: DTK_E_ARG)
// The next runs of a one-document batch walk a slice of a stream: open_slice (0: the window ends where the stream
// does) and the record to start from (null: the stream's beginning).  batch_cut: the last run's cut block, behind finish().
int batch_set_slice(dtk_batch *b, uint32_t open_slice, const DtkLaneState *carry);
int batch_cut(dtk_batch *b, DtkStreamCut *out);
// dtk_slice.cpp.  batch_set_slice_request: what the slice's next download computes; slice_outputs: enqueues it on the
// download stream (dtk_batch_download_begin, behind the event list).  Behind dtk_batch_result_host:
//   batch_render_out  kPlainBytes: the page-locked bytes
//   batch_pos_out     kPosBytes: the bytes and the trailer block behind them (DTK_E_CAPACITY / DTK_E_IRREGULAR as it says)
//   batch_offs_out    offs: the page-locked arrays (DTK_E_CAPACITY / DTK_E_IRREGULAR as the trailer says); the blocked
//                     pointers are null where the plain arrays stand in, and the other way round
//   batch_sens_out    sens: the page-locked rows (DTK_E_CAPACITY / DTK_E_IRREGULAR as its own trailer says)
struct SsView {
  const DtkSensTrailer *t;
  const uint32_t *tok_end, *tse;
  const uint64_t *bstart, *bend;
  const int64_t *rstart, *rend;
};
struct SoView {
  const DtkOffsTrailer *t;
  const int64_t *rstart, *rend, *sent;
  const uint32_t *words;
  const DtkOffBlock64 *heads;
  const uint32_t *ttok, *tsent;
};
inline void batch_set_slice_request(dtk_batch *b, const SliceRequest &q) { b->slice.req = q; }
int slice_outputs(dtk_batch *b);
int batch_render_out(dtk_batch *b, const uint8_t **out, uint64_t *out_len);
int batch_pos_out(dtk_batch *b, const uint8_t **out, const DtkPosTrailer **trailer);
int batch_offs_out(dtk_batch *b, SoView *o);
int batch_sens_out(dtk_batch *b, SsView *o);
inline uint64_t blocks_of(uint64_t tokens) { return (tokens + 63) / 64; }  // blocks of 64 tokens

// The DTK_R_* arrays the last run wrote: DTK_NO_RUNE_OFFSETS / DTK_NO_BYTE_OFFSETS leave theirs alone.
inline uint32_t run_fields(const dtk_batch *b) {
  uint32_t f = ~0u;
  if (b->last_flags & DTK_NO_RUNE_OFFSETS) f &= ~(uint32_t)(DTK_R_TOK_RUNE | DTK_R_TOK_RUNE16 | DTK_R_TOK_RUNE_BLK);
  if (b->last_flags & DTK_NO_BYTE_OFFSETS) f &= ~(uint32_t)(DTK_R_TOK_BYTE | DTK_R_TOK_BYTE_BLK | DTK_R_SENTENCES);
  return f;
}

// The last run's output arrays, into the fields of the same names of `o` (dtk_result_view, DtkCompactArgs or
// DtkExactArgs); what the run does not write is null.  The kernels' arguments also get the renderer's bookkeeping,
// which any of the offsets-only flags leaves out.
template <class A>
void set_outputs(const dtk_batch *b, A &o) {
  const uint32_t f = run_fields(b);
  o.tok_off = b->d_tok_off; o.sent_off = b->d_sent_off; o.text_off = b->d_text_off;
  o.tok_rstart = (f & DTK_R_TOK_RUNE) ? b->d_rstart : nullptr; o.tok_rend = (f & DTK_R_TOK_RUNE) ? b->d_rend : nullptr;
  o.tok_bstart = (f & DTK_R_TOK_BYTE) ? b->d_bstart : nullptr; o.tok_bend = (f & DTK_R_TOK_BYTE) ? b->d_bend : nullptr;
  o.sent = b->d_sent; o.text_tok_end = b->d_ttok; o.text_sent_end = b->d_tsent;
  if constexpr (!std::is_same<A, dtk_result_view>::value) {
    const bool ro = (b->last_flags & (DTK_OFFSETS_ONLY | DTK_NO_RUNE_OFFSETS | DTK_NO_BYTE_OFFSETS)) != 0;
    o.tok_sbefore = ro ? nullptr : b->d_sbefore; o.text_s_end = ro ? nullptr : b->d_ts_end;
    o.doc_ns = ro ? nullptr : b->d_doc_ns;
  }
}

#pragma GCC visibility pop
