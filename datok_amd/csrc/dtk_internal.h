// dtk_internal.h -- structures shared by the host side and the gfx950 kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define DTK_FIRSTBIT 0x80000000u   // datok.go:43
#define DTK_SECONDBIT 0x40000000u  // datok.go:44
#define DTK_RESTBIT 0x3fffffffu    // datok.go:45
#define DTK_EOT 4u                 // matrix.go:13
#define DTK_WINDOW 1024u           // matrix.go:365
#define DTK_WINDOW_BYTES 4104u     // more bytes than 1024 runes can have: the window has overflowed for certain

// ---- symbol stream entry (uint16 per input byte), written by the symbolise kernel
//   [10:0]  sigma index a           (sigmaASCII[c] / sigma[c] / identity, matrix.go:421-435)
//   [13:11] bytes of the rune that starts at this byte (Go DecodeRune width, 1..4); 0: no rune starts here
//   [15:14] class: 0 rune<256, 1 rune==EOT, 2 rune>=256 in sigma (ok=true), 3 not in sigma (ok=false)
// (an entry with width 0 and the epsilon symbol is what the lean walk feeds itself for an epsilon iteration)
#define DTK_SYM_MASK 0x7FFu
#define DTK_SYM_MAX 2047u
#define DTK_SYM_W_SHIFT 11
#define DTK_SYM_CLS_SHIFT 14
#define DTK_SYM_WIDTH(e) (((uint32_t)(e) >> DTK_SYM_W_SHIFT) & 7u)
#define DTK_SYM_IS_START(e) (DTK_SYM_WIDTH(e) != 0u)
// the general walk's per-lane window of the symbol stream in LDS: entries, and u16 per row (72 B)
#define DTK_WIN 32u
#define DTK_WIN_ROW 36u
// ---- the stream in memory: one BYTE per input byte where the model's entries fit a code table (DtkSigmaDev::n_codes:
// the shipped models have some 170 symbols and 200 distinct entries), else the 16-bit entries themselves.  A code
// is an index into `lut` (256 entries); DTK_SYM_CONT = no rune starts here.  Half the stream's traffic -- it was 44 %
// of what a batch moves -- and the lean walk's windows (codes) in 40 instead of 72 bytes of LDS per lane.  The code of a
// byte below 128 is the byte itself (upload() in dtk_model.cpp; k_symbolize copies those).
#define DTK_SYM_CONT 0xFFu
#ifndef DTK_WIN8
#define DTK_WIN8 32u  // positions in a lean-walk row of codes (a multiple of 16; the row has 8 bytes more: 40 B)
#endif
// The lean walk's row over a stream of 16-bit entries (a model with more than 255 of them): DTK_WIN16 entries, a
// multiple of 8; DTK_ROW_PAD16 bytes between the lanes' rows (a multiple of 8); DTK_WALK_OCC16 waves per SIMD the
// first pass is built for -- what the LDS of a wave admits.  Build knobs of the recorded A/B; what
// they must keep is checked at compile time (WinChecked, dtk_walk_core.h).
#ifndef DTK_WIN16
#define DTK_WIN16 16u
#endif
#ifndef DTK_ROW_PAD16
#define DTK_ROW_PAD16 0u
#endif
#ifndef DTK_WALK_OCC16
#define DTK_WALK_OCC16 7
#endif
// Elements behind max_bytes that a batch's stream (and text) buffers are allocated with (dtk_batch_create): the lean
// loop reads up to a row behind the batch's last byte (the static_asserts behind WinEntries, dtk_walk_core.h)
#define DTK_STREAM_PAD 256u
struct DtkSym {
  const void *base;     // uint8_t codes if lut, else uint16_t entries
  const uint16_t *lut;  // [256] entry of a code (lut[DTK_SYM_CONT] has width 0), or null
};
#ifdef __HIP__
__device__ __forceinline__ uint32_t dtk_sym_entry(const DtkSym &S, uint64_t i) {
  return S.lut ? (uint32_t)S.lut[static_cast<const uint8_t *>(S.base)[i]] : (uint32_t)static_cast<const uint16_t *>(S.base)[i];
}
__device__ __forceinline__ bool dtk_sym_is_start(const DtkSym &S, uint64_t i) {
  return S.lut ? static_cast<const uint8_t *>(S.base)[i] != DTK_SYM_CONT
               : DTK_SYM_IS_START(static_cast<const uint16_t *>(S.base)[i]);
}
#endif

// ---- walk output: event bitmaps over cursor positions.  Position p (0..len) of document d, which starts at
// input byte `off`, is bit  G = off + d + p  (one position more than the document has bytes, so the ranges of
// consecutive documents follow each other without sharing a bit).  One bitmap per kind of event, `bit_words`
// 32-bit words each, kind k at bits + k * bit_words; all cleared before a run.  Order of the calls at one cursor
// position: SEOT, TEOT (the cursor only reaches the byte behind an EOT by consuming it, which fires SentenceEnd /
// TextEnd at once, matrix.go:593-600), END (a token that ends there: double array only, which keeps its window),
// SEPS.  START is no call: it marks the first byte of the token whose END is the next END bit.
// The final SentenceEnd / TextEnd (matrix.go:683-691) are two bits of the document's tail word, with the
// cursor they fire at:  doc_tail[d] = cursor << 2 | 1 (SentenceEnd) | 2 (TextEnd).
// The walk collects END / START / SEPS bits in LDS (one set of bitmaps per wave, covering the positions of its
// 64 chunk lanes) and writes whole words out at the end: one scattered byte store per event cost a third of the
// pipeline's throughput (each reaches memory as its own partial-sector write).
enum { EVB_END = 0, EVB_START = 1, EVB_SEPS = 2, EVB_TEOT = 3, EVB_SEOT = 4, EVB_KINDS = 5 };
#define DTK_EV_BIT(off, d) ((uint64_t)(off) + (uint64_t)(d))
#define DTK_TAIL_S 1u
#define DTK_TAIL_E 2u
// LDS words per kind for a wave of 64 chunk lanes of `chunk` bytes: 64 * (chunk + 1) positions + alignment slack
#define DTK_LDS_BIT_WORDS(chunk) (2u * (chunk) + 8u)
#define DTK_LDS_BIT_CHUNK_MAX 256u  // larger chunks write their bits straight to memory

// flags of one queued cursor position inside the compaction (bit order = call order)
#define EV_S_EOT 0x01u
#define EV_E_EOT 0x02u
#define EV_TOK_END 0x04u
#define EV_S_EPS 0x08u
#define EV_S_EOF 0x20u
#define EV_E_EOF 0x40u

// per-document status (mirrors DTK_ST_* of datok_gpu.h)
#define ST_WINDOW_OVERFLOW 1u
#define ST_EMPTY_TEXT 2u
#define ST_BAD_MODEL 4u
#define ST_IRREGULAR 8u
#define ST_STEP_LIMIT 16u
#define ST_BAD_OFFSET 64u  // Token call with its offset behind its buffer (the reference panics when it prints the surface)
#define ST_INTERNAL 32u  // the walk's counts and the compaction disagree (a bug, never expected)

struct DtkSigmaDev {
  const uint16_t *ascii;  // [256] symbol per rune < 256 (identity pre-filled, matrix.go:289-293)
  const uint32_t *runes;  // sorted runes of the sigma map (matrix.go:301)
  const uint16_t *syms;   // their symbols
  uint32_t n_runes;
  uint32_t identity;
  // code table (n_codes != 0: the stream holds codes)
  uint32_t n_codes;
  const uint16_t *code_entry;  // [256] code -> entry
  const uint8_t *code_lt256;   // [256] rune < 256 -> code (one byte wide below 128, two from 128 on)
  const uint8_t *code_runes;   // [n_runes] sigma rune >= 256 in its UTF-8 width -> code
  uint8_t code_ident[5];       // [w] a rune of w bytes that is not in the sigma (identity, ok = false)
  uint8_t code_fffd1;          // an invalid byte (U+FFFD, one byte wide) if U+FFFD is in the sigma
};

enum { DTK_KIND_MATRIX = 0, DTK_KIND_DA = 1 };

// Device table handed to the walk kernels.
// The walk's lookup count (a statistic) is added up in 32 counters a cache line apart, picked by block id: one
// counter took 2048 adds to one address from the waves of a batch as they finished, 5 us at the end of the walk.
#define DTK_STEP_STRIPES 32u
#define DTK_TOTALS_BYTES (128u + DTK_STEP_STRIPES * 128u)  // a batch's totals block + the counters behind it

// A slice of one long stream (dtk_stream_run): the window [0, S + T) is walked as one document, and
// the verified start record of the first lane behind S -- the reference's exact loop state at its first rewind at or
// behind S -- is the cut.  Calls in front of it are the slice's; the next slice, whose window begins S bytes later,
// starts from the record.  Written by k_stream_cut (dtk_streamcut.hip), cleared with the totals block.
struct DtkStreamCut {
  uint32_t p, t, aux, flags;  // the carry: a DtkLaneState, its position relative to the next window (cut - S)
  uint32_t cut;               // window-relative position of the cut; 0xFFFFFFFF: the walk closed the document in front of S
  uint32_t valid;             // 1: the kernel ran
  // The one lane that walks from a carried record takes the writer for new (LANE_F_FRESH), so its DTK_ST_EMPTY_TEXT may
  // be wrong: its status is kept out of the document's and reported here, with the position its walk ended at
  // (0xFFFFFFFF: the document's end) -- the host decides the bit from the calls up to there and the stream's own state.
  uint32_t walker_status, walker_end;
};
// The totals block at the head of a batch's accumulators, with its page-locked mirror on the host.
struct DtkTotalsDev {
  uint64_t n_tok, n_sent, n_text, n_flagged;  // the scan: tokens, sentence ints, texts, documents with a status
  uint64_t unused_4[2];
  uint64_t invalid_epoch;              // k_symbolize: number of the last run that saw an invalid UTF-8 byte
  uint32_t any_irregular, any_eot;     // the compaction: some document is ST_IRREGULAR / is left to k_compact_eot
  uint32_t n_bad[4];                   // documents to repair after the first pass / after each device-side round
  uint64_t render_total;               // host copy only: bytes of the rendering (dtk_results.cpp)
  uint64_t to_host_epoch;              // k_to_host: number of the run whose results it copied
  struct DtkStreamCut cut;             // k_stream_cut: where a stream's slice ends and what the next one starts from
};
static_assert(sizeof(struct DtkTotalsDev) == DTK_TOTALS_BYTES - DTK_STEP_STRIPES * 128u, "the block is 128 bytes");
// the scan (k_scan3_tiles / k_scan3_mid) writes totals[0..3]; k_compact*, k_to_host read totals[0..2]
static_assert(offsetof(struct DtkTotalsDev, n_tok) == 0 && offsetof(struct DtkTotalsDev, n_sent) == 8 &&
              offsetof(struct DtkTotalsDev, n_text) == 16 && offsetof(struct DtkTotalsDev, n_flagged) == 24,
              "the scan's four totals are the first four words");
// k_symbolize clears the block in 16-byte units and leaves one word of one unit alone
static_assert(offsetof(struct DtkTotalsDev, invalid_epoch) % 16 == 0 &&
              offsetof(struct DtkTotalsDev, any_irregular) == offsetof(struct DtkTotalsDev, invalid_epoch) + 8,
              "invalid_epoch and the two flags share a 16-byte unit");
// the striped lookup counters behind the block (DtkWalkArgs::steps): stripe i
static inline uint64_t *dtk_step_stripe(struct DtkTotalsDev *t, uint32_t i) { return (uint64_t *)(t + 1) + 16u * i; }

struct DtkTableDev {
  int kind;
  // matrix: state-major rows, cell (t, a) at tab[t*stride + a]; column 0 is all
  // zero (the a == 0 guard of matrix.go:459).  cell = target | nontoken flag in
  // the top bit.  States are renumbered so that exactly the states 1..n_eps
  // have an epsilon arc (the probe of matrix.go:442 becomes a compare).
  // double array: {base, check} pairs as in the file (datok.go:56-59); bit 30 of
  // base (unused upstream, masked by getBase, datok.go:271-273) caches "this
  // index has an epsilon arc" so the probe of datok.go:876 needs no extra load.
  const void *tab;
  uint32_t entry_bytes;  // matrix: 2 or 4 plain, 4 or 8 fused (dtk_model.cpp pick_encoding); 8 (double array pairs)
  uint32_t stride;       // matrix: cells per row
  uint32_t n_states;     // matrix: highest state id
  uint32_t n_eps;        // matrix: states 1..n_eps have an epsilon arc
  uint32_t start;        // image of the reference's state 1
  uint32_t fused;        // matrix: cells with fused epsilon+rune entries, of entry_bytes 4 or 8 (FusedCell32 / FusedCell64, dtk_walk_core.h)
  uint32_t ident_guard;  // identity symbol if arcs on `unknown` exist, else 0xFFFFFFFF
  uint32_t da_dense;     // 1: a double-array tokenizer whose transitions were laid out as a (fused) matrix at load
  uint32_t da_len;       // double array: pairs
  uint32_t da_size;      // array[1].check & RESTBIT (datok.go:333-335)
  uint32_t da_base1;     // device base word of index 1
  uint32_t epsilon, unknown, identity;
  uint32_t lean16;       // a stream of 16-bit entries is walked by the lean loop too (0: test hook GENERAL16, the general loop)
};

// ---- speculative chunk lanes
#define LANE_F_SENT 1u     // sentenceEnd (matrix.go:360)
#define LANE_F_TEXT 2u     // textEnd (matrix.go:363)
#define LANE_F_OK 4u       // sticky ok (matrix.go:352)
#define LANE_F_DROPPED 8u  // the lane produced an event outside its window
#define LANE_F_IDLE 16u
#define LANE_F_FRESH 32u   // start records only: the writer behind this record is new (a slice's carried record, which
                           // the compaction takes for a document's start: no token yet, in the text or at all)
enum { PLAN_OFF = 0, PLAN_CHAINED = 1, PLAN_LAST = 2 };

// Loop state at a "sync point" = right after the reference rewinds its window
// (matrix.go:537-543, 608-627): nothing else survives a rewind.
struct DtkLaneState {
  uint32_t p;      // byte position in the document; 0xFFFFFFFF = none / ran to EOF
  uint32_t t;      // automaton state
  uint32_t aux;    // double array: device base word of t
  uint32_t flags;  // LANE_F_*
};
struct DtkLanePlan {
  uint32_t stop;   // stop at the first sync point at or behind this position
  uint32_t wend;   // events are stored up to here (the next lane's start position)
  uint32_t mode;   // PLAN_*
  uint32_t pad;
};
struct DtkLaneCount {
  uint32_t tok, sent, text;  // Token calls, ints of the sentence list, TextEnd calls
  uint32_t status;
  // for compacting a long document in segments (k_seg_*): SentenceEnd calls, and the lane's last
  // TextEnd fired by an EOT: its position (0xFFFFFFFF = none) and the lane's Token calls before it
  uint32_t sev, e_pos, e_tok;
  uint32_t pad;
};
struct DtkSpecArgs {
  uint32_t n_lanes;
  uint32_t chunk, warm;             // chunk size C and warm-up overlap W in bytes
  const uint32_t *lane_doc;         // lane -> document
  const uint32_t *chunk_off;        // document -> first lane (n_docs + 1)
  struct DtkLaneState *lane_start;  // record each lane starts from
  struct DtkLaneState *lane_end;    // where it stopped
  struct DtkLanePlan *lane_plan;
  struct DtkLaneCount *lane_cnt;
  uint32_t *first_bad;              // per document: first chunk without a linked successor
  uint32_t *fail_lane;              // per document: first lane that missed its successor's record
  const uint32_t *redo_from;        // repair rounds: first lane to redo per document, or null
  const uint8_t *text;              // input bytes (k_spec_start: whitespace-guided warm-up), or null
  uint32_t warm_extend;             // move the warm-up start back to the previous blank, at most this many bytes (0: off)
  uint32_t first_repair;            // repair rounds: 1 in the round that follows the first pass
  uint32_t lds_words;               // LDS bitmap words per kind for one wave (0: event bits go straight to memory)
  // A repair round enqueued ahead of time (device-side repair): its kernels return at once unless *go != 0
  // (the number of documents the previous verification found broken); null: run.
  const uint32_t *go;
};

struct DtkWalkArgs {
  struct DtkSym sym;        // symbol stream, one entry per input byte
  const uint64_t *doc_off;  // n_docs + 1
  uint32_t n_docs;
  uint32_t *bits;           // event bitmaps (EVB_KINDS x bit_words words), zero-filled
  uint32_t bit_words;
  uint32_t *doc_tail;       // per document, zero-filled
  uint32_t *status;         // per document, OR-ed
  uint64_t *tok_cnt, *sent_cnt, *text_cnt;  // per document: what the writer would have collected
  unsigned long long *steps;  // global lookup counter
  uint32_t step_factor;     // cap = step_factor * (len + 2) lookups per document
  // A slice of a stream (one document): the record its walk starts from in place of {0, start state} -- every lane
  // whose chunk does not begin behind it has this record -- or null; and for the walk with one lane per document,
  // which has no lane records, the open end: it stops at the first sync point at or behind open_stop (0: walks to
  // EOF) and leaves the record there in *open_fin.
  const struct DtkLaneState *init_rec;
  uint32_t open_stop;
  struct DtkLaneState *open_fin;
};

// k_stream_cut (dtk_streamcut.hip): ends document 0 of a one-document batch at its cut.
struct DtkStreamCutArgs {
  uint32_t slice;                       // S: the cut is the start record of lane ceil(S / chunk); 0: the stream's last slice, no cut
  const struct DtkLaneState *init_rec;  // the record the slice started from, or null (the stream's first slice)
  uint32_t chunk, n_lanes;              // chunk 0: one lane per document, the record is *open_fin and nothing lies behind it
  const struct DtkLaneState *lane_start;
  struct DtkLaneCount *lane_cnt;
  const struct DtkLaneState *open_fin;
  uint32_t *bits;
  uint32_t bit_words;
  uint32_t *doc_tail, *status;
  uint64_t *tok_cnt, *sent_cnt, *text_cnt;
  const uint32_t *skip_if;              // documents still to repair: the kernel does nothing unless this is 0 (null: run)
  struct DtkStreamCut *out;
};

struct DtkCompactArgs {
  const uint8_t *text;
  const uint32_t *rs_bits;  // bit g: input byte g starts a rune (k_symbolize)
  const uint64_t *doc_off;
  uint32_t n_docs;
  const uint32_t *bits;     // event bitmaps of the walk
  uint32_t bit_words;
  const uint32_t *doc_tail;
  uint32_t *status;
  uint32_t flags;           // DTK_NEWLINE_AFTER_EOT
  int kind;                 // matrix / double array (EOT rewind rule differs)
  // pass 1 output: per document counts (tokens, sentence ints, texts)
  uint64_t *tok_off, *sent_off, *text_off;  // n_docs+1; counts in [d], scanned in place
  // pass 2 output
  int32_t *tok_rstart, *tok_rend;
  uint32_t *tok_bstart, *tok_bend;
  int32_t *sent;
  uint32_t *text_tok_end, *text_sent_end;
  // for the renderer: SentenceEnd calls (of the document) before each Token / TextEnd call, and per document
  uint32_t *tok_sbefore, *text_s_end, *doc_ns;
  const uint64_t *totals;   // [0..2] tokens, sentence ints, texts (written by the scan)
  uint64_t tok_cap, sent_cap, text_cap;
  // Long documents are compacted in segments of DTK_SEG_LANES chunk lanes (matrix walk with chunk
  // lanes only; null = one wave per document): segment -> document / first lane / lanes
  const uint32_t *seg_doc, *seg_lane0, *seg_nl;
  uint32_t n_segs;
  const uint32_t *chunk_off;              // document -> first lane
  const struct DtkLaneState *lane_start;  // sync points = where segments begin
  const struct DtkLaneCount *lane_cnt;
  struct DtkSegSum *seg_sum;              // k_seg_sum: what a segment adds
  struct DtkSegIn *seg_in;                // k_seg_scan: the carries a segment starts with
  uint32_t *doc_seq;                      // k_seg_scan: 1 = this long document must be compacted sequentially
  uint32_t *any_irregular;                // set to 1 if a document is flagged ST_IRREGULAR (the host then runs the exact pass)
  uint32_t *any_eot;                      // set to 1 by k_compact_plain if a document is left to k_compact_eot
  const uint32_t *skip_if;                // documents still to repair: the pass does nothing unless this is 0 (null: run)
};

#define DTK_SEG_LANES 64u
// what the lanes of one segment add up to (k_seg_sum)
struct DtkSegSum {
  uint32_t tok, sent, text, sev;  // Token calls, sentence ints, TextEnd calls, SentenceEnd calls
  uint32_t runes;                 // rune starts in the segment's positions
  uint32_t e_pos;                 // last EOT TextEnd inside (0xFFFFFFFF: none) ...
  uint32_t e_tok, e_runes;        // ... Token calls / rune starts of the segment before it
};
// the state k_compact starts a segment with: everything that precedes it in the document
struct DtkSegIn {
  uint32_t tok, sent, text, sev, runes;
  uint32_t e_pos, e_tok, e_runes;  // last EOT TextEnd before the segment (absolute), 0xFFFFFFFF: none
};

// ---- the exact pass: documents whose call order the position-indexed event bytes cannot express
// (ST_IRREGULAR: the double array consuming one EOT twice after a backtrack, datok.go:916-926 +
// 1019-1030; a third epsilon SentenceEnd at one cursor, matrix.go:573-576) are walked again by one
// lane each, in the reference's own order, writing their rows of the result arrays directly and
// listing their calls (dtk_call of datok_gpu.h) for closure replays.
struct DtkCall { uint32_t kind; int32_t a; uint32_t b, c; };
struct DtkExactArgs {
  struct DtkSym sym;
  const uint8_t *text;
  const uint64_t *doc_off;
  uint32_t n;               // documents to walk
  const uint32_t *docs;     // their ids
  uint32_t pass;            // 0: count the calls (n_calls[i]); 1: write rows and calls
  uint32_t *n_calls;        // [n]
  const uint64_t *call_off; // [n + 1], pass 1: calls of docs[i] at calls[call_off[i] ..)
  struct DtkCall *calls;
  uint32_t *status;
  uint32_t flags;           // DTK_NEWLINE_AFTER_EOT
  uint32_t step_factor;
  const uint64_t *tok_off, *sent_off, *text_off;  // CSR rows (sized by the walk's counts)
  int32_t *tok_rstart, *tok_rend;
  uint32_t *tok_bstart, *tok_bend;
  int32_t *sent;
  uint32_t *text_tok_end, *text_sent_end;
  uint32_t *tok_sbefore, *text_s_end, *doc_ns;    // renderer bookkeeping (may be null)
};

// NewTokenWriter's byte output on the device (dtk_render.hip)
struct DtkRenderArgs {
  const uint8_t *text;
  const uint64_t *doc_off;
  uint32_t n_docs;
  uint32_t flags;  // TOKENS 1, SENTENCES 2, TOKEN_POS 4, SENTENCE_POS 8
  const uint64_t *tok_off, *sent_off, *text_off;  // CSR rows per document
  uint64_t n_tok, n_sent, n_text;
  const int32_t *rstart, *rend, *sent;
  const uint32_t *bstart, *bend, *sbefore;  // per token
  const uint32_t *ttok, *tsent, *ts_end;    // per text: tokens / sentence ints / SentenceEnd calls up to its TextEnd
  const uint32_t *doc_ns;                   // SentenceEnd calls per document
  struct DtkSym sym;                        // symbol stream; base non-null only if the batch has invalid UTF-8 bytes
  // workspace
  uint64_t *A, *P, *Q;           // exclusive scans: surface bytes, position digits (n_tok+1), sentence digits (n_sent+1)
  uint64_t *blkA, *blkP, *blkQ;  // per-tile sums
  uint64_t *ns_off;              // n_docs+1
  uint64_t *tx_base, *tx_stream, *tx_pos, *tx_sent;  // n_text+1
  // output
  uint64_t *out_off;  // n_docs+1
  uint8_t *out;
  uint64_t out_total;
};

// Results straight into page-locked host memory from the batch's own stream (k_to_host): the sizes of the offset
// arrays are only known on the device when the copies have to be enqueued, so a copy engine cannot be asked ahead of
// time -- a kernel can: it reads the totals and streams the rows over the link with 16-byte stores.
#define DTK_TOHOST_MAX 14
struct DtkToHostArgs {
  const void *src[DTK_TOHOST_MAX];
  void *dst[DTK_TOHOST_MAX];           // mapped page-locked host memory
  uint64_t bytes[DTK_TOHOST_MAX];      // size in bytes (count_from < 0), else bytes per element
  int32_t count_from[DTK_TOHOST_MAX];  // < 0: fixed size; 0..2: totals[count_from] elements
  uint64_t cap[DTK_TOHOST_MAX];        // elements source and destination hold (count_from >= 0)
  uint32_t n;
  const uint64_t *totals;              // device totals block (scan3)
  const uint32_t *skip_if;             // documents still to repair: nothing is copied unless this is 0 (null: copy)
  uint64_t *done;                      // device word: set to the run's epoch when the copy was made
  uint64_t epoch;
};

// DTK_R_TOK_RUNE_BLK / DTK_R_TOK_BYTE_BLK (k_pack_blk): one pair of offset arrays into its blocked form
// (include/datok_gpu.h, dtk_off_block).  The byte offsets are below 2^31: both pairs are read as int32.
struct DtkPackBlkPair {
  const int32_t *start, *end;  // n each
  uint32_t *words;             // n
  void *heads;                 // ceil(n / 64) dtk_off_block, 16-byte aligned
  uint32_t *flag;              // device word, cleared in front of the launch: 1 is ORed in if a block does not fit
};
struct DtkPackBlkArgs {
  struct DtkPackBlkPair pair[2];
  uint32_t n_pairs;
  uint32_t span;  // largest maximum - minimum a segment of a block may have (65 535)
  uint64_t n;     // tokens
};

// DTK_R_EVENT_LIST (dtk_evlist.hip): the set bits of SEPS | TEOT | SEOT as rows {position, kinds} with a CSR over
// documents (include/datok_gpu.h).  Global bits are below 2^32 (the walk's EventSink counts them in 32 bits too).
#define DTK_EVL_K_SEOT 1u  // DTK_EVL_* of datok_gpu.h
#define DTK_EVL_K_TEOT 2u
#define DTK_EVL_K_SEPS 4u
struct DtkEvListArgs {
  const uint32_t *bits;     // event bitmaps of the walk (EVB_KINDS x bit_words words)
  uint32_t bit_words;
  uint32_t n_docs;
  const uint64_t *doc_off;  // n_docs + 1, on the device
  uint64_t n_bits;          // doc_off[n_docs] + n_docs: bits at or behind it belong to no document
  uint32_t n_tiles;         // dtk_evlist_tiles(n_bits, bit_words)
  uint32_t cap;             // rows evl_pos / evl_kind / evl_bit hold; a larger total writes no row
  uint32_t *tile_base;      // n_tiles: counts, then their exclusive scan
  uint32_t *count;          // device word: the total
  uint32_t *evl_off;        // n_docs + 1
  uint32_t *evl_pos;        // cap
  uint8_t *evl_kind;        // cap
  uint32_t *evl_bit;        // cap, device only: a row's global bit (what k_evl_rows searches)
};

// DTK_R_SENTENCES (dtk_sentences.hip): the batch's sentences as rows (include/datok_gpu.h, dtk_sentence_view), read off
// the event bitmaps and gathered from the token rows.  Global bits are below 2^32, as for the event list.
struct DtkSentencesArgs {
  const uint32_t *bits;     // event bitmaps of the walk (EVB_KINDS x bit_words words)
  uint32_t bit_words;
  uint32_t n_docs;
  const uint64_t *doc_off;  // n_docs + 1, on the device
  uint64_t n_bits;          // doc_off[n_docs] + n_docs: bits at or behind it belong to no document
  uint32_t n_tiles;         // dtk_sentences_tiles(n_bits, bit_words)
  uint32_t cap;             // rows the arrays below hold; a larger total writes nothing
  const uint64_t *tok_off, *text_off;         // n_docs + 1 each
  const uint32_t *tok_bstart, *tok_bend;      // the run's token rows
  const int32_t *tok_rstart, *tok_rend;       // null: the run wrote no rune offsets, sen_rstart / sen_rend stay unwritten
  const uint32_t *text_tok_end;               // the run's text rows
  uint64_t text_cap;                          // rows text_sen_end holds
  uint32_t *tile_base;      // n_tiles: a tile's summary word, then its first row
  uint32_t *tile_in;        // n_tiles: f in front of the tile
  uint32_t *count;          // device word: the total
  uint32_t *sen_bit, *sen_doc, *sen_first;    // cap each, device only: a row's global bit, document, first token
  uint64_t *sen_off;        // n_docs + 1
  uint32_t *sen_tok_end, *sen_bstart, *sen_bend;  // cap each
  int32_t *sen_rstart, *sen_rend;                 // cap each
  uint32_t *text_sen_end;   // text_cap
};

// A stream slice's writer bytes in the position-free modes (dtk_streamrender.hip, dtk_stream_set_render): the one
// document's tokens merged with its event list, on the download stream behind k_evl_*.
struct DtkStreamRenderArgs {
  uint32_t bits;               // DTK_TOKENS | DTK_SENTENCES
  uint32_t with_tail;          // the stream's last slice: the tail word's SentenceEnd / TextEnd follow
  const uint8_t *text;         // the window
  uint32_t text_len;
  struct DtkSym sym;           // base non-null only if the run saw invalid UTF-8
  uint64_t n_tok;
  const uint32_t *tok_bstart, *tok_bend;
  const uint32_t *evl_pos;     // the list of document 0 (evl_off[0] == 0)
  const uint8_t *evl_kind;
  const uint32_t *evl_count;   // device word: its length
  uint32_t evl_cap;            // rows the list's arrays hold; a longer list renders nothing (out_len = ~0)
  const uint32_t *doc_tail;
  uint32_t tok_tiles, ent_tiles;  // dtk_streamrender_tiles(n_tok) / (evl_cap)
  uint64_t *tok_base, *ent_base;  // tok_tiles / ent_tiles: tile sums, then their exclusive scans
  uint64_t *ew;                // evl_cap + 1: exclusive scan of the entries' bytes
  uint8_t *out;                // cap bytes, 16-byte aligned, filled with '\n' in front of the launch
  uint64_t cap;                // nothing is written at or behind it
  uint64_t *out_len;           // device word: the exact length
};

// The same in a mode with TOKEN_POS / SENTENCE_POS (dtk_streampos.hip, dtk_stream_set_position_render).  The writer's
// state in front of and behind a slice: what crosses a cut (token_writer.go:38-42; pos.back() == posC whenever pos is
// not empty, and the integers already collected are bytes of a line the host holds).
struct DtkPosCarry {
  int64_t posC;                            // Go's int
  uint32_t sentB, init, pos_nonempty, sent_nonempty;
};
// what goes home behind the bytes in one block
struct DtkPosTrailer {
  uint64_t out_len;                        // ~0: the list did not fit its arrays, nothing was rendered
  uint64_t open_pos_len, open_sent_len;    // the fragments of the text open at the cut: behind out, in this order
  uint64_t splice_pos, splice_sent;        // offsets into out, ~0: none
  struct DtkPosCarry carry_in, carry_out;
  uint32_t flags;                          // 1: a token with rend == 0 under NEWLINE_AFTER_EOT (the literal rule would fire again)
  uint32_t pad;
};
// the scanning blocks' results, for the kernels behind them
struct DtkPosHdr {
  uint64_t tot[3];                         // bytes of all tokens: surfaces, position integers, sentence integers
  uint64_t ent_tot;                        // bytes of all entries
  uint64_t head_w;                         // sentence integers of SentenceEnd calls in front of the first token and TextEnd
  uint32_t head_n, n_te;                   // their number; TextEnd entries of the list
  uint32_t flags, pad;
};
struct DtkStreamPosArgs {
  uint32_t bits;               // the five writer bits, one of TOKEN_POS / SENTENCE_POS among them
  uint32_t with_tail;
  uint32_t is_matrix;          // the window start follows a TextEnd fired by an EOT (matrix.go:601)
  uint32_t first;              // window byte where the slice's calls begin
  const uint8_t *text;
  uint32_t text_len;
  struct DtkSym sym;           // base non-null only if the run saw invalid UTF-8
  uint64_t n_tok;
  const uint32_t *tok_bstart, *tok_bend;
  const uint32_t *evl_pos;
  const uint8_t *evl_kind;
  const uint32_t *evl_count;
  uint32_t evl_cap;
  const uint32_t *doc_tail;
  uint32_t tok_tiles, ent_tiles;
  const struct DtkPosCarry *carry_in;   // device: the predecessor's carry_out
  struct DtkPosCarry *carry_out;        // device: another slot
  // workspace (dtk_streampos_ws gives the sizes)
  struct DtkPosHdr *hdr;
  uint64_t *ent_base;          // ent_tiles: tile sums, then their exclusive scans (twice: counts, then bytes)
  uint64_t *cnt;               // evl_cap + 1: SentenceEnd calls (low word) and TextEnd entries (high word) in front of an entry
  uint64_t *ew;                // evl_cap + 1: exclusive scan of the entries' bytes
  uint64_t *ent_pre;           // evl_cap: an entry's bytes in front of a token on its cursor
  uint32_t *te_idx;            // evl_cap: the entry of the c-th TextEnd
  uint64_t *seg_pos, *seg_sent;   // evl_cap + 2 each, per text of the slice: where its lines begin in the output
  uint64_t *seg_pw0;           // ... the position-integer scan at its first token
  int64_t *seg_sw0;            // ... the sentence-integer scan there (less the head's integers for text 0)
  int64_t *tile_sum, *tile_in; // tok_tiles: a tile's segmented sum of rune counts; posC in front of the tile
  uint32_t *tile_flag;         // tok_tiles: the tile has a token that begins a text
  uint64_t *w_base;            // 3 * tok_tiles: tile sums of the three weights, then their exclusive scans
  int64_t *rstart, *rend;      // n_tok
  int32_t *tok_v;              // n_tok: runes a token adds to posC (less one where the newline rule fires)
  uint32_t *tok_len;           // n_tok: runes of the surface
  uint32_t *tok_meta;          // n_tok: SentenceEnd calls that read this token's end | begins a text << 30 | sentB << 31
  uint32_t *tok_seg;           // n_tok: TextEnd entries in front of the token
  uint32_t *w_in;              // 3 * n_tok: a weight's exclusive scan inside its tile
  uint8_t *out;                // cap bytes, filled with '\n' in front of the launch
  uint64_t cap;                // nothing is written at or behind it
  struct DtkPosTrailer *trailer;
};

// The writer's rune offsets and sentence list of a slice as arrays (dtk_streamoffs.hip, dtk_stream_set_offsets): what a
// NewTokenWriter with TOKEN_POS | SENTENCE_POS collects in pos[] / sent[] during the slice's calls.  The front of the
// chain is position rendering's (dtk_streampos_front.h): `front` holds its inputs and the part of the workspace it
// reads (dtk_streamoffs_ws), with bits = TOKEN_POS | SENTENCE_POS and the run's NEWLINE_AFTER_EOT.
struct DtkOffBlock64 { int64_t base0, base1; uint32_t brk, reserved; };  // dtk_off_block64 of datok_gpu.h
struct DtkOffsTrailer {
  uint64_t n_tok;                          // ~0: the list did not fit its arrays, nothing was computed
  uint64_t n_sent, n_text;                 // ints pushed to sent[], TextEnd calls: beyond a capacity, the array is cut short
  struct DtkPosCarry carry_in, carry_out;
  uint32_t flags;                          // 1: a token with rend == 0 under NEWLINE_AFTER_EOT
  uint32_t blk_fail;                       // 1: a segment of a block spans more than `span` (k_so_pack64)
};
struct DtkStreamOffsArgs {
  struct DtkStreamPosArgs front;           // (rstart / rend: the plain arrays, n_tok each; out / cap / trailer unused)
  uint64_t *sent_base;                     // workspace, tok_tiles: a tile's sentence ints, then their exclusive scan
  uint32_t *sent_in;                       // workspace, n_tok: a token's place among its tile's sentence ints
  int64_t *sent;                           // sent_cap
  uint64_t sent_cap, text_cap;             // nothing is written at or behind them
  uint32_t *text_tok_end, *text_sent_end;  // text_cap each
  uint32_t blocked;                        // pack tok_rstart / tok_rend into words + heads
  uint32_t span;                           // largest maximum - minimum a segment of a block may have (65 535)
  uint32_t *words;                         // n_tok
  struct DtkOffBlock64 *heads;             // ceil(n_tok / 64), 8-byte aligned
  struct DtkOffsTrailer *trailer;
};

// The sentences of a slice as rows (dtk_streamsens.hip, dtk_stream_set_sentences), behind the offsets chain of the same
// slice: `front` is that chain's, with its workspace as the chain left it (tok_meta, rstart / rend, hdr, te_idx, the
// writer's carry_out).  What crosses a cut is the row that is open there.
struct DtkSenCarry {                       // dtk_stream_sen_carry of datok_gpu.h
  uint32_t open, reserved;
  uint64_t bstart, bend;                   // stream byte offsets: start of its first token, end of its last so far
  int64_t rstart, rend;                    // the writer's rune offsets of the same two
};
struct DtkSensTrailer {
  uint64_t n_tok;                          // ~0: the list did not fit its arrays, nothing was computed
  uint64_t n_sen, n_text;                  // rows closed by this slice's calls, TextEnd calls: beyond a capacity, the array is cut short
  uint64_t firsts;                         // tokens of the slice that begin a sentence (the kernels' own)
  struct DtkSenCarry carry_in, carry_out;
  uint32_t flags, pad;                     // 1: a token with rend == 0 under NEWLINE_AFTER_EOT
};
struct DtkStreamSensArgs {
  struct DtkStreamPosArgs front;
  uint64_t base;                           // stream offset of window byte 0
  const struct DtkSenCarry *carry_in;      // device: the predecessor's carry_out
  struct DtkSenCarry *carry_out;           // device: another slot
  uint64_t *first_base;                    // workspace, tok_tiles: a tile's sentence-first tokens, then their exclusive scan
  uint64_t *first_mask;                    // workspace, ceil(n_tok / 64): which tokens of a wave's 64 begin a sentence
  uint64_t sen_cap, text_cap;              // nothing is written at or behind them
  uint32_t *sen_tok_end;                   // sen_cap each
  uint64_t *sen_bstart, *sen_bend;
  int64_t *sen_rstart, *sen_rend;
  uint32_t *text_sen_end;                  // text_cap
  struct DtkSensTrailer *trailer;
};

#ifdef __cplusplus
extern "C" {
#endif
#define DTK_STREAMSENS_EVENTS 5   // one in front of the unit's four launches and one behind each
int dtk_launch_streamsens(const struct DtkStreamSensArgs *args, void *stream, void **events);  // events: null, or that many hipEvent_t
uint64_t dtk_streamsens_ws(struct DtkStreamSensArgs *args, uint64_t *ws);  // as dtk_streampos_ws, the unit's own two arrays
#define DTK_STREAMOFFS_EVENTS 11  // one in front of the chain's ten launches and one behind each
int dtk_launch_streamoffs(const struct DtkStreamOffsArgs *args, void *stream, void **events);  // events: null, or that many hipEvent_t
uint64_t dtk_streamoffs_ws(struct DtkStreamOffsArgs *args, uint64_t *ws);  // as dtk_streampos_ws
int dtk_launch_streampos(const struct DtkStreamPosArgs *args, void *stream);
int dtk_pos_trailer_check(const struct DtkPosTrailer *t, uint64_t cap);  // DTK_OK, DTK_E_CAPACITY or DTK_E_IRREGULAR
uint64_t dtk_streampos_ws(struct DtkStreamPosArgs *args, uint64_t *ws);  // lays the workspace out (ws null: the size only), in 64-bit words
uint32_t dtk_streamrender_tiles(uint64_t n);
int dtk_launch_streamrender(const struct DtkStreamRenderArgs *args, void *stream);
uint32_t dtk_evlist_tiles(uint64_t n_bits, uint32_t bit_words);
int dtk_launch_evlist(const struct DtkEvListArgs *args, void *stream);
uint32_t dtk_sentences_tile_bits(void);  // cursor positions per tile of dtk_sentences.hip
uint32_t dtk_sentences_tiles(uint64_t n_bits, uint32_t bit_words);
int dtk_launch_sentences(const struct DtkSentencesArgs *args, void *stream);
int dtk_launch_to_host(const struct DtkToHostArgs *args, void *stream);
int dtk_launch_pack_r16(const int32_t *rs, const int32_t *re, uint32_t *out, uint64_t n, void *stream);
int dtk_launch_pack_blk(const struct DtkPackBlkArgs *args, void *stream);
// launchers (dtk_symbolize / dtk_walk / dtk_repair / dtk_compact .hip); stream is a hipStream_t
int dtk_launch_symbolize(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs,
                         uint64_t total, const struct DtkSigmaDev *sig, void *sym, int padded,
                         const uint32_t *blk_doc, unsigned long long *n_invalid, uint32_t *rs_bits,
                         uint32_t *ev_bits, uint32_t bit_words, void *acc, uint64_t acc_bytes, uint64_t epoch, void *stream);
#ifndef DTK_SYM_BLOCK_BYTES
#define DTK_SYM_BLOCK_BYTES 4096u  // input bytes per symbolise block (blk_doc granularity)
#endif
int dtk_launch_walk(const struct DtkTableDev *tab, const struct DtkWalkArgs *args, void *stream);
// The launches of the speculative walk (dtk_launch_spec).  The first pass of a run is START, LINK, WALK, VERIFY or
// START_WALK, LINK_VERIFY, then FIX unless the scan carries its step; a repair round (spec->redo_from set) is
// SPREAD_RESET, dtk_launch_redo_clear, LINK, WALK, VERIFY, FIX (dtk_run.cpp: first_pass, repair_round).
enum DtkSpecStage {
  DTK_SPEC_START = 0,         // k_spec_start: the lanes' start records (first pass, split shape)
  DTK_SPEC_LINK = 1,          // k_spec_link (first pass, split shape; every repair round)
  DTK_SPEC_WALK = 2,          // k_spec_walk: the chunk walk (first pass, split shape; every repair round)
  DTK_SPEC_VERIFY = 3,        // k_spec_verify (first pass, split shape; every repair round)
  DTK_SPEC_FIX = 4,           // k_spec_fix: counts the broken documents (first pass, unless the scan does it; every repair round)
  DTK_SPEC_SPREAD_RESET = 5,  // k_redo_spread, k_redo_reset (repair rounds only, first of the round)
  DTK_SPEC_START_WALK = 6,    // k_spec_both: start records and chunk walk in one launch (first pass only, fused shape)
  DTK_SPEC_LINK_VERIFY = 7,   // k_spec_verify with its link step (first pass only, fused shape)
};
int dtk_launch_spec(const struct DtkTableDev *tab, const struct DtkWalkArgs *args,
                    const struct DtkSpecArgs *spec, enum DtkSpecStage stage, uint32_t cmp_mask, uint32_t *redo_out,
                    uint32_t *n_bad, void *stream);
// (the stages that do not walk, dtk_repair.hip: LINK, VERIFY, LINK_VERIFY, FIX, SPREAD_RESET)
int dtk_launch_spec_check(const struct DtkWalkArgs *args, const struct DtkSpecArgs *spec, enum DtkSpecStage stage,
                          uint32_t cmp_mask, uint32_t *redo_out, uint32_t *n_bad, void *stream);
int dtk_launch_redo_clear(const struct DtkWalkArgs *args, const struct DtkSpecArgs *spec, void *stream);
int dtk_launch_stream_cut(const struct DtkStreamCutArgs *args, void *stream);
// which kernels dtk_launch_compact launches: for the documents without an EOT call, for those with one, or both
enum DtkCompactWhich { DTK_COMPACT_PLAIN = 1, DTK_COMPACT_EOT = 2, DTK_COMPACT_BOTH = 3 };
int dtk_launch_compact(const struct DtkCompactArgs *args, uint32_t small_max, const uint32_t *big_docs, uint32_t n_big,
                       int which, void *stream);
int dtk_launch_exact(const struct DtkTableDev *tab, const struct DtkExactArgs *args, void *stream);
int dtk_launch_seg_prepare(const struct DtkCompactArgs *args, const uint32_t *doc_seg0, void *stream);
int dtk_launch_render(const struct DtkRenderArgs *args, int stage, void *stream);
uint32_t dtk_render_tiles(uint64_t n);
uint64_t dtk_render_ws(struct DtkRenderArgs *args, uint64_t *ws);  // as dtk_streampos_ws, the eight spare words included
int dtk_launch_clear2(void *a, uint64_t a_bytes, void *b, uint64_t b_bytes, void *stream);
// Up to this many documents the row offsets come from one launch of independent 256-document tiles (k_scan3_tiles,
// which can also do k_spec_fix's per-document step); above it from three launches.  Every tile adds up the counts
// of all tiles below it, so the reads grow with the square of the document count.  The scan stage of one batch alone
// (stage events, 64-byte documents, median of 40 runs, us; in brackets scan + fix stages: the three-launch path needs
// k_spec_fix's launch beside it, and an empty stage still measures 5.2), tiles against three launches:
//    8 192 documents  16.7 (21.8)  against  19.5 (26.1)
//   16 384            25.9 (31.1)           19.6 (26.2)
//   32 768            44.5 (49.7)           20.2 (26.8)
//   65 536            83.8 (89.0)           20.1 (26.7)
// The crossover lies between the first two sizes (near 12 000 documents by a straight line between them): the limit
// stays at the largest size measured at which the tiles win.
#ifndef DTK_SCAN_TILES_MAX_DOCS
#define DTK_SCAN_TILES_MAX_DOCS 8192u
#endif
int dtk_launch_scan3(const uint64_t *ca, const uint64_t *cb, const uint64_t *cc, uint64_t *a, uint64_t *b,
                     uint64_t *c, uint32_t n_docs, uint64_t *totals, const uint32_t *status, uint64_t *ws,
                     const struct DtkSpecArgs *fix_spec, uint32_t *redo_out, uint32_t *n_bad, const uint32_t *skip_if,
                     void *stream);
#ifdef __cplusplus
}
#endif
