/*
 * datok_gpu.h -- C-ABI of the MI355X batch tokenizer (libdatok_gpu.so).
 *
 * This is the drop-in boundary for the one hot path of KorAP/Datok: the
 * matrix / double-array FSA walk behind
 *     LoadTokenizerFile            (fomafile.go:452-484)
 *     Tokenizer.Transduce          (matrix.go:340-342, datok.go:769-771)
 *     Tokenizer.TransduceTokenWriter (matrix.go:348-698, datok.go:781-1135)
 *     TokenWriter / NewTokenWriter (token_writer.go:27-33, 36-175)
 * A cgo shim binds exactly these entry points; the C++ and
 * Python host mirrors in this repo sit on the same ABI.  Plain pointers and
 * sizes only: no torch, no HIP types in any signature (a HIP stream is passed
 * as void*).
 *
 * Every compute entry point runs on the GPU.  There is no CPU fallback: if no
 * HIP device is usable the calls return DTK_E_NO_DEVICE.
 */
#ifndef DATOK_GPU_H
#define DATOK_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (negative); dtk_strerror() renders them ---- */
enum {
  DTK_OK = 0,
  DTK_E_IO = -1,        /* cannot open / read (matrix.go:215-219) */
  DTK_E_FORMAT = -2,    /* not gzip, bad magic, bad version, short file (matrix.go:253-334) */
  DTK_E_NO_DEVICE = -3, /* no usable HIP device */
  DTK_E_HIP = -4,       /* a HIP runtime call failed; dtk_last_hip_error() has the text */
  DTK_E_ARG = -5,       /* invalid argument */
  DTK_E_MODEL = -6,     /* model outside device limits (>= 2048 symbols, epsilon cycle, ids out of range),
                           or a Foma net ParseFoma rejects (fomafile.go:159-167,283-310) */
  DTK_E_CAPACITY = -7,  /* batch larger than the dtk_batch was created for */
  DTK_E_STATE = -8,     /* call order (e.g. result requested before a run) */
  DTK_E_NOMEM = -9,     /* host allocation failed */
  DTK_E_IRREGULAR = -10 /* dtk_stream_run: a slice needs the exact pass (calls that are not in position order, which
                           only crafted models produce); tokenize the text as one document (dtk_transduce*, dtk_batch) */
};

/* ---- Bits, token_writer.go:17-25 (same values) ---- */
enum {
  DTK_TOKENS = 1,
  DTK_SENTENCES = 2,
  DTK_TOKEN_POS = 4,
  DTK_SENTENCE_POS = 8,
  DTK_NEWLINE_AFTER_EOT = 16,
  DTK_SIMPLE = 3,
  /* dtk_batch_run only (not a reference bit): the caller wants the offset arrays only; the
   * per-token bookkeeping of dtk_batch_render_* is not written (a render then returns DTK_E_STATE) */
  DTK_OFFSETS_ONLY = 256,
  /* dtk_batch_run only, each implies DTK_OFFSETS_ONLY: a caller that reads one kind of token offsets does not pay for
   * the other (the compaction otherwise writes four 32-bit words per token where the north star's arrays have two;
   * tok_rstart / tok_rend resp. tok_bstart / tok_bend then come back NULL).  The closure replay and the device
   * renderer need the byte offsets. */
  DTK_NO_BYTE_OFFSETS = 512,
  DTK_NO_RUNE_OFFSETS = 1024
};

/* ---- per-document status bits: inputs on which the reference panics or
 *      that the device representation cannot express.  Offsets of a document
 *      with status != 0 are out of contract. ---- */
enum {
  DTK_ST_WINDOW_OVERFLOW = 1, /* > 1024 buffered runes: matrix.go:365/406 index panic */
  DTK_ST_EMPTY_TEXT = 2,      /* SentenceEnd/TextEnd with no token in the text:
                                 token_writer.go:108,135,145 panic in position modes */
  DTK_ST_BAD_MODEL = 4,       /* walk left the table */
  DTK_ST_IRREGULAR = 8,       /* internal: calls not in position order; such a document is re-walked by the
                                 exact pass (dtk_result_view.n_exact) and never reported with this bit */
  DTK_ST_STEP_LIMIT = 16,     /* safety cap on lookups hit */
  DTK_ST_INTERNAL = 32,       /* internal consistency check failed (a bug; never expected) */
  DTK_ST_BAD_OFFSET = 64      /* a Token call whose offset lies behind its buffer (after a hard fail with the
                                 epsilon slot behind the token start, e.g. "x ....\n\n" at the end of a document):
                                 string(buf[offset:]) panics in the reference when surfaces are printed
                                 (token_writer.go:85,93); in position-only modes it yields start > end */
};

typedef struct dtk_model dtk_model;
typedef struct dtk_batch dtk_batch;

/* ---- token offsets as 16-bit blocks (DTK_R_TOK_RUNE_BLK, DTK_R_TOK_BYTE_BLK): 4.25 B per token instead of 8, for
 *      documents of any length.  Tokens are taken in the batch-wide order of the result arrays (the order tok_off
 *      indexes); block j holds the tokens [64j, 64j + 64).  Inside one text the offsets never decrease from one token
 *      to the next, and 64 consecutive tokens span little (the reference's window holds at most 1024 runes between two
 *      rewinds); the large jumps are the resets at a text or document boundary.  A block therefore has one break:
 *        brk   = the smallest lane l >= 1 of the block with start[64j + l] < end[64j + l - 1], or 64 if there is none
 *        base0 = the minimum over every start and end of the lanes < brk
 *        base1 = the minimum over the lanes >= brk, or 0 if brk == 64
 *        word[i] = (start[i] - base) | (end[i] - base) << 16   with base = lane < brk ? base0 : base1
 *      (both halves unsigned 16-bit; the -1 of token_writer.go:66-68 lands in a base).  The last block of a batch is
 *      partial: lanes behind the last token take part in nothing.  A batch in which some segment of some block spans
 *      more than 65 535 does not get this form: the pointers come back NULL and the 32-bit arrays are delivered in
 *      their place. ---- */
typedef struct { int32_t base0, base1; uint32_t brk, reserved; } dtk_off_block;
/* The decoders: inline for C, cgo and C++ callers; libdatok_gpu.so also exports the two under the same names for
 * callers that bind symbols (ctypes, ...) -- the library's own unit defines DTK_BLK_DECODER away to emit them. */
#ifndef DTK_BLK_DECODER
#define DTK_BLK_DECODER static inline
#endif
DTK_BLK_DECODER int32_t dtk_blk_start(const uint32_t *words, const dtk_off_block *heads, uint64_t i) {
  const dtk_off_block *h = heads + (i >> 6);
  return ((uint32_t)(i & 63u) < h->brk ? h->base0 : h->base1) + (int32_t)(words[i] & 0xFFFFu);
}
DTK_BLK_DECODER int32_t dtk_blk_end(const uint32_t *words, const dtk_off_block *heads, uint64_t i) {
  const dtk_off_block *h = heads + (i >> 6);
  return ((uint32_t)(i & 63u) < h->brk ? h->base0 : h->base1) + (int32_t)(words[i] >> 16);
}

/* ---- devices ---- */
int dtk_device_count(void);
int dtk_set_device(int device);          /* device used by subsequent loads / batches of this thread */
const char *dtk_strerror(int code);
const char *dtk_last_hip_error(void);

/* Test hook.  The library never reads the environment; the code paths it otherwise picks by model, batch shape or
 * history (general loop instead of the lean one, 16-bit stream entries, the double array's pairs instead of its
 * dense layout, two-launch first pass, ...) can be forced through this call so that the test suite runs over each
 * of them.  key: the name in dtk_model.cpp's table, with or without the "DATOK_" prefix the tests' environment
 * variables carry (datok_amd/_lib.py forwards those); value: an integer as text (NULL = 1).  No switch changes a
 * result.  Set before the models / batches it should affect are created. */
int dtk_debug_configure(const char *key, const char *value);

/* Test accessor, read-only: what the symbolise kernel wrote in the batch's last run.  Waits for that run, then copies
 * home
 *   entries[total]: one 16-bit entry per input byte,
 *       bits 10..0   the symbol of the rune that starts at this byte, as the model FILE numbers it (sigmaASCII[c] /
 *                    sigma[c] / identity, matrix.go:421-435; 0 for a net without an identity symbol),
 *       bits 13..11  the bytes of that rune (Go DecodeRune width, 1..4); 0: no rune starts here, and the other bits
 *                    of such an entry mean nothing,
 *       bits 15..14  class: 0 rune < 256, 1 rune == U+0004 (EOT), 2 rune >= 256 in the sigma (ok = true),
 *                    3 not in the sigma (ok = false),
 *     whatever the stream's format on the device (one-byte codes are translated through the model's code table) and
 *     the device table's column order (columns are translated back to the file's symbols);
 *   rune_start_words[(total + 31) / 32]: bit g set: input byte g starts a rune;
 *   *saw_invalid: 1 if the run met an invalid UTF-8 byte (it prints as U+FFFD), else 0.
 * Any of the three may be NULL.  DTK_E_ARG before the batch's first run and between a new input and its run. */
int dtk_batch_debug_stream(dtk_batch *b, uint16_t *entries, uint32_t *rune_start_words, uint32_t *saw_invalid);

/* ---- model: replaces LoadTokenizerFile (fomafile.go:452-484), LoadMatrixFile
 *      (matrix.go:214-231), LoadDatokFile (datok.go:600-617).  gunzip, sniff
 *      "MATOK"/"DATOK", parse, build the device tables.  Immutable afterwards,
 *      shareable between batches and threads. ---- */
int dtk_model_load(const char *path, dtk_model **out);
int dtk_model_load_mem(const void *gz_bytes, size_t n, dtk_model **out); /* ParseMatrix/ParseDatok on a gzip blob */
void dtk_model_free(dtk_model *m);
/* Both loaders also accept a gzip'd Foma text net ("##foma-net ..."): LoadFomaFile + Automaton.ToMatrix
 * (fomafile.go:56-450, matrix.go:30-99), i.e. what the reference's tests build their tiny tokenizers with.
 * dtk_foma_to_matok is `datok convert` without --double-array (cmd/datok.go:50-70): the same conversion
 * followed by MatrixTokenizer.Save (matrix.go:107-210) into a gzip image (*out, free with dtk_free).
 * Host only: needs no device.
 * dtk_foma_to_datok is `datok convert --double-array`: Automaton.ToDoubleArray (datok.go:82-238, Mizobuchi et al. 2000
 * with the xCheckSkipNiu search) followed by DaTokenizer.Save (datok.go:485-596).  The reference lays the states out
 * in the order Go's map iteration hands it their symbols (fomafile.go:488-495) -- two runs give two arrays; here the
 * symbols are taken in ascending order, so the image is one the reference can produce, not a particular one. */
int dtk_foma_to_matok(const void *gz_bytes, size_t n, void **out, size_t *out_n);
int dtk_foma_to_datok(const void *gz_bytes, size_t n, void **out, size_t *out_n);
const char *dtk_model_type(const dtk_model *m); /* Tokenizer.Type(): "MATOK" / "DATOK" (matrix.go:102, datok.go:252) */

typedef struct {
  int32_t kind;          /* 0 matrix, 1 double array */
  int32_t epsilon, unknown, identity, final_state, sigma_count;
  uint32_t state_count;  /* matrix: stateCount; double array: array[1].check */
  uint64_t array_len;    /* matrix: u32 cells; double array: {base,check} pairs */
  uint32_t n_eps_states; /* states with an epsilon arc */
  uint32_t max_eps_chain;/* longest path of epsilon arcs */
  uint32_t entry_bytes;  /* device table cell size.  Matrix, and a double array laid out as one (dense_states != 0):
                          * 4 = fused cells with 15-bit state ids (the lean loop's table), 8 = fused cells of 64 bits
                          * (32 767 states and more), 2 or 4 = plain cells (the test hooks' layouts; 4 also for a table
                          * beyond the 64-bit cells' 32-bit byte offset).  Double array walked as pairs: 8 */
  uint64_t device_bytes; /* HBM held by the model */
  uint32_t unknown_used; /* 1 if any state has an arc on the unknown symbol */
  uint32_t dense_states; /* double array only: its states, if its transitions were laid out as a matrix on the
                          * device at load (entry_bytes is then 4 or 8, see there); 0: the {base, check} pairs are walked */
  uint32_t stream_codes; /* distinct symbol-stream entries of the model if they fit a byte (the stream is then one
                          * code per input byte); 0: more than 255 of them, the stream holds the 16-bit entries
                          * themselves.  The format of the stream only: which loop walks it is lean_walk */
  uint32_t lean_walk;    /* 1: dtk_batch_run walks this model with the lean loop -- fused cells (entry_bytes 4 or 8 of a
                          * matrix, or of a double array with dense_states != 0) and unknown_used == 0, over codes or
                          * over 16-bit entries alike; 0: the general loop, at about half the walk rate (an arc on
                          * `unknown`, plain cells, a double array walked as pairs, the test hook GENERAL16) */
} dtk_model_info;
int dtk_model_get_info(const dtk_model *m, dtk_model_info *out);
/* The same answer for an image that is not loaded: parses gz_bytes and decides the device layout exactly as
 * dtk_model_load_mem does (device_bytes: what the model would hold), and touches no device -- like dtk_foma_to_matok
 * it runs on a machine without a GPU.  What a grammar maintainer's CI asks after an update: which table, which loop. */
int dtk_model_info_mem(const void *gz_bytes, size_t n, dtk_model_info *out);

/* ---- batch: one data-parallel TransduceTokenWriter over n_docs documents.
 *      Each document is one reference call with a fresh writer
 *      (matrix.go:348 / datok.go:781).  A dtk_batch owns its device buffers
 *      (sized once at creation) and one HIP stream; no allocation happens in
 *      dtk_batch_run. ---- */
int dtk_batch_create(uint64_t max_bytes, uint32_t max_docs, dtk_batch **out);
void dtk_batch_free(dtk_batch *b);

/* Host input: text = concatenated documents, doc_off[n_docs+1] byte offsets
 * (doc_off[0] == 0).  Copies to the device on the batch's stream. */
int dtk_batch_set_input(dtk_batch *b, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs);
/* Device-resident input (e.g. a torch tensor's data_ptr): no copy is made, the
 * buffers must stay valid until the run has been synchronised. */
int dtk_batch_set_input_device(dtk_batch *b, const void *d_text, const void *d_doc_off,
                               uint32_t n_docs, uint64_t total_bytes);

/* Walk strategy.  chunk_bytes = 0: one lane per document.  Otherwise documents are
 * cut into chunks of chunk_bytes; every chunk is walked by its own lane from a
 * speculative start found warm_bytes earlier, and a check pass proves that each
 * lane arrived exactly where its successor started (mismatches are repaired, the
 * result is always exact).  0xFFFFFFFF (the default) picks the chunk size from
 * the batch size.  warm_bytes defaults to 8 (the start then moves back to the previous blank, see below). */
int dtk_batch_set_chunking(dtk_batch *b, uint32_t chunk_bytes, uint32_t warm_bytes);

/* A speculative start that falls inside a long blank-free token (a URL) would invent
 * token ends; the start is therefore moved back from chunk - warm_bytes to the previous
 * blank, by at most max_bytes (default 240; 0 = keep the fixed distance, which tests use
 * to force mispredictions).  Speed only: the result is exact either way. */
int dtk_batch_set_warm_extend(dtk_batch *b, uint32_t max_bytes);

/* Launches the whole path on the batch's stream (asynchronous):
 * symbolise -> walk -> count -> scan -> compact.  flags: DTK_NEWLINE_AFTER_EOT
 * is the only bit that changes the numbers (token_writer.go:66-68); DTK_OFFSETS_ONLY
 * skips what only the device renderer needs. */
int dtk_batch_run(const dtk_model *m, dtk_batch *b, uint32_t flags);
int dtk_batch_sync(dtk_batch *b);
/* Lend the batch HIP streams instead of the one it owns: `compute` for its kernels (NULL: keep), `upload` for the
 * copies of dtk_batch_set_input (NULL: on the compute stream).  The batches of a dtk_pipeline share one of each: the
 * HIP runtime has four hardware queues, streams that share one serialise, and a pipeline of any depth then needs three
 * (uploads, kernels, downloads).  The streams must outlive the batch's use of them. */
int dtk_batch_set_streams(dtk_batch *b, void *compute, void *upload);
int dtk_batch_done(dtk_batch *b); /* 1 if everything dtk_batch_run enqueued has finished, 0 if not; never blocks */
void *dtk_batch_stream(dtk_batch *b); /* hipStream_t, for event timing by the caller */

/* Optional per-stage timing with HIP events recorded on the batch's stream
 * around each kernel of dtk_batch_run (no host synchronisation is added).
 * dtk_batch_stage_ms() synchronises and returns the milliseconds of the last
 * run: [0] clears [1] symbolise [2] start records [3] link [4] chunk walk (or
 * the one-lane-per-document walk) [5] verify [6] fix [7] scan [8] compaction.
 * That is the first pass as four launches; as two (the fused shape): [2] and
 * [3] are empty, [4] is start records + walk, [5] is link + verify. */
#define DTK_N_STAGES 9
int dtk_batch_set_profiling(dtk_batch *b, int enable);
int dtk_batch_stage_ms(dtk_batch *b, float ms[DTK_N_STAGES]);

/* Totals of the last run (synchronises). */
typedef struct {
  uint32_t n_docs;
  uint64_t n_bytes;
  uint64_t n_tokens;      /* Token calls */
  uint64_t n_sent;        /* ints in the flat sentence list (token_writer.go:78,108) */
  uint64_t n_texts;       /* TextEnd calls */
  uint64_t n_flagged;     /* documents with status != 0 */
  uint64_t walk_steps;    /* table lookups performed by the walk kernels (warm-ups included) */
  uint32_t n_lanes;       /* lanes the walk ran on */
  uint32_t chunk_bytes;   /* chunk size used (0: one lane per document) */
  uint32_t repair_rounds; /* speculation repair rounds (normally 0) */
} dtk_totals;
int dtk_batch_totals(dtk_batch *b, dtk_totals *out);

/*
 * Result arrays of the last run.  CSR over documents:
 *   tokens of doc d:  [tok_off[d], tok_off[d+1])
 *     tok_rstart/tok_rend : rune offsets relative to the current text, exactly the
 *                           pos[] pairs of token_writer.go:72-81
 *     tok_bstart/tok_bend : byte offsets relative to the document (surface slices)
 *   sentence ints of d: [sent_off[d], sent_off[d+1])  -- the flat sent[] list of
 *                           token_writer.go:75-79,104-109 (start of first token after a
 *                           sentence/text end, end of last token at a SentenceEnd)
 *   texts of d:        [text_off[d], text_off[d+1])   -- one per TextEnd:
 *     text_tok_end[i]  = tokens of the document emitted before it
 *     text_sent_end[i] = sentence ints emitted before it
 *   status[d]          = DTK_ST_* bits
 * Pointers are DEVICE pointers owned by the batch, valid until the next run.
 */
/* One call of the reference into the TokenWriter, for documents walked by the exact pass (below):
 * kind 0 = Token(offset, buf): a = byte position of buf[0], b = of buf[offset], c = end of buf
 *          (document relative; b > c only in DTK_ST_BAD_OFFSET documents);
 * kind 1 = SentenceEnd(a);  kind 2 = TextEnd(a) -- a is the int the reference passes
 *          (matrix.go:575,597,600,684,691: buffc; datok.go:1015,1026,1119,1127: 0, :1023: buffc). */
typedef struct { uint32_t kind; int32_t a; uint32_t b, c; } dtk_call;

typedef struct {
  const uint64_t *tok_off, *sent_off, *text_off; /* n_docs+1 each */
  const int32_t *tok_rstart, *tok_rend;
  const uint32_t *tok_bstart, *tok_bend;
  const int32_t *sent;
  const uint32_t *text_tok_end, *text_sent_end;
  const uint32_t *status;
  /* Raw walk output, for replay into TokenWriter closures: one bitmap per kind of event over the cursor
   * positions p = 0..len of every document.  Position p of document d is bit DTK_EVENT_BIT(doc_off[d], d) + p;
   * bitmap k (DTK_EVB_*) is ev_bits[k * ev_words .. (k + 1) * ev_words).  Calls at one cursor position are
   * fired in the order SEOT, TEOT, END (the token whose first byte is the last START bit below), SEPS.  The
   * final SentenceEnd / TextEnd (matrix.go:683-691) are in doc_tail[d] = cursor << 2 | DTK_TAIL_S | DTK_TAIL_E.
   * The k-th END bit of a document belongs to its k-th token (tok_bstart / tok_bend). */
  const uint32_t *ev_bits;
  uint64_t ev_words;
  const uint32_t *doc_tail;
  /* The exact pass.  The event bytes order the calls by cursor position.  Two constructs of the
   * reference break that order (or put two calls on one bit): the double array consuming one EOT rune twice (it keeps its window
   * over an EOT, datok.go:1019-1030, so a later backtrack, :916-926, re-reads it: SentenceEnd /
   * TextEnd, then a Token that ends BEFORE them, then both again), and more than two epsilon
   * SentenceEnds at one cursor (matrix.go:573-576 has no limit).  No shipped model does either on
   * any test corpus; a document that does is walked again by a single lane in the reference's own
   * order, which writes its rows of the arrays above (bit-exact like all others) and lists its
   * calls here.  For the n_exact documents exact_doc[i] (ascending) a replay must use
   * calls[exact_off[i] .. exact_off[i+1]) instead of the event bitmaps. */
  uint32_t n_exact;
  const uint32_t *exact_doc;
  const uint64_t *exact_off; /* n_exact + 1 */
  const dtk_call *calls;
  /* DTK_R_TOK_RUNE16 (host results only): (uint16_t)tok_rstart[i] | (uint32_t)(uint16_t)tok_rend[i] << 16, or NULL */
  const uint32_t *tok_r16;
  /* DTK_R_TOK_RUNE_BLK / DTK_R_TOK_BYTE_BLK (host results only): the rune resp. byte offsets in blocks of 64 tokens,
   * one word per token and one dtk_off_block per block (above); NULL when not delivered */
  const uint32_t *tok_rblk;
  const dtk_off_block *tok_rblk_head;
  const uint32_t *tok_bblk;
  const dtk_off_block *tok_bblk_head;
  /* DTK_R_EVENT_LIST (host results only; NULL when not delivered): the sparse events of a closure replay as a list
   * instead of bitmaps.  A pure function of the bitmaps above: document d has one entry for every cursor p in
   * 0..len(d) at which bit DTK_EVENT_BIT(doc_off[d], d) + p is set in any of DTK_EVB_SEPS, DTK_EVB_TEOT,
   * DTK_EVB_SEOT; evl_kind says in which of them (DTK_EVL_* below).  END and START are not listed: the k-th END bit
   * of a document is at cursor tok_bend[k], and its START bit at tok_bstart[k].
   *   evl_off   n_docs + 1: the entries of document d are [evl_off[d], evl_off[d + 1])
   *   evl_pos   cursor position, document relative, 0..len, strictly ascending within a document
   *   evl_kind  DTK_EVL_* bits, never 0
   * The replay of document d merges its tokens (cursor tok_bend[k], first byte tok_bstart[k], or dtk_blk_end /
   * dtk_blk_start on the blocked byte offsets) with its entries by position; at one cursor the calls fire in the
   * order SEOT, TEOT, the Token ending there, SEPS.  doc_tail[d] comes last, as with the bitmaps.  The int arguments
   * are those of the bitmap replay: the rune count since the window start, which a Token and (matrix only) a TEOT
   * move to their cursor (include/datok.hpp, detail::replay_list).  Documents listed in exact_doc are replayed from
   * `calls`; their entries follow the same definition and are not used. */
  const uint32_t *evl_off;
  const uint32_t *evl_pos;
  const uint8_t *evl_kind;
} dtk_result_view;
int dtk_batch_result_device(dtk_batch *b, dtk_result_view *out);
/* status words of the first n documents, copied to the caller's array */
int dtk_batch_status_host(dtk_batch *b, uint32_t *status, uint32_t n);
/* The results on the host.  The reference hands every token to a host closure (matrix.go:528,569,677 -> w.Token,
 * token_writer.go:72-88); here the arrays come over in one chain of asynchronous copies into page-locked memory owned
 * by the batch, on a HIP stream of their own (the batch's stream and the upload direction of the link stay free).
 *   dtk_batch_set_result_fields: which arrays a caller wants (DTK_R_*, default all): a caller that only reads the
 *       rune offsets moves 1.1 B per input byte instead of 2.8; one that replays the events into closures needs
 *       DTK_R_EVENTS | DTK_R_TOK_BYTE | DTK_R_CSR | DTK_R_STATUS.
 *   dtk_batch_download_begin: completes the run like dtk_batch_totals, enqueues the copies and returns at once
 *       (dtk_pipeline uses it to bring slice i home under the walk of slice i + 1 and the upload of slice i + 2).
 *   dtk_batch_result_host: begins the download if nobody has, waits for it, and returns host pointers (valid until the
 *       batch's next run / free); arrays that were not selected are NULL. */
enum {
  DTK_R_CSR = 1,       /* tok_off, sent_off, text_off */
  DTK_R_TOK_RUNE = 2,  /* tok_rstart, tok_rend */
  DTK_R_TOK_BYTE = 4,  /* tok_bstart, tok_bend */
  DTK_R_SENT = 8,      /* sent */
  DTK_R_TEXTS = 16,    /* text_tok_end, text_sent_end */
  DTK_R_STATUS = 32,   /* status */
  DTK_R_EVENTS = 64,   /* ev_bits, doc_tail (doc_tail also comes with DTK_R_EVENT_LIST) */
  DTK_R_ALL = 127,
  /* tok_r16: the rune offsets of a token as the two halves of one 32-bit word -- start in the low half, end in the
   * high half, both int16 -- half the bytes of tok_rstart / tok_rend on the link (the download is the longer leg of a
   * host-to-host pass: 1.2 B per input byte against 1 B of upload).  Offsets never exceed a document's length, so the
   * narrow form exists when no document of the batch is longer than 32 767 bytes; for a batch with a longer one
   * tok_r16 comes back NULL and tok_rstart / tok_rend are delivered in its place.  Not part of DTK_R_ALL. */
  DTK_R_TOK_RUNE16 = 128,
  /* with any of the above: the selected arrays leave for the host inside dtk_batch_run -- a kernel behind the
   * compaction reads the row counts on the device and streams the rows into the batch's page-locked buffers, so no
   * host round trip stands between the walk and the copy.  dtk_batch_result_host then finds them there (a run that
   * needed a repair round, larger arrays or the exact pass copies again by itself). */
  DTK_R_EAGER = 256,
  /* tok_rblk + tok_rblk_head resp. tok_bblk + tok_bblk_head: the rune resp. byte offsets as 16-bit blocks
   * (dtk_off_block above; decode with dtk_blk_start / dtk_blk_end), packed on the download stream in front of their
   * copies.  Host results only, not part of DTK_R_ALL nor of the eager copy.  If a block of the batch does not fit 16
   * bits the pair's pointers come back NULL and its 32-bit arrays are delivered in their place (the caller looks at
   * which pointer it got, as with tok_r16).  DTK_R_TOK_RUNE16 | DTK_R_TOK_RUNE_BLK asks for the narrowest form that
   * applies: tok_r16 for a batch of documents of up to 32 767 bytes, the blocked form for any other. */
  DTK_R_TOK_RUNE_BLK = 512,
  DTK_R_TOK_BYTE_BLK = 1024,
  /* evl_off + evl_pos + evl_kind + doc_tail: what a closure replay needs of the event bitmaps beside the token
   * offsets, as a list (dtk_result_view above) -- about one 5-byte entry per sentence where the bitmaps cost five
   * bits per input byte.  Compacted from the bitmaps on the download stream in front of its copies.  Host results
   * only, not part of DTK_R_ALL nor of the eager copy; works with every run flag, and may be selected together with
   * DTK_R_EVENTS.  A closure replay then needs DTK_R_EVENT_LIST | DTK_R_TOK_BYTE (or DTK_R_TOK_BYTE_BLK) | DTK_R_CSR |
   * DTK_R_STATUS.  The copies are enqueued for n_sent + n_texts entries, which bounds the count for regular documents;
   * dtk_batch_result_host looks at the true count behind the download and copies again if that was too few. */
  DTK_R_EVENT_LIST = 2048,
  /* the sentence table (dtk_sentence_view below, read with dtk_batch_sentences_host): built from the event bitmaps and
   * the token rows on the download stream in front of its copies and brought home with the other fields, about 20 B
   * per sentence.  Like DTK_R_EVENT_LIST not part of DTK_R_ALL nor of the eager copy.  A run with DTK_NO_BYTE_OFFSETS
   * has no table (it is keyed on tok_bend): the bit is then ignored.  (4096 stays an unknown bit.) */
  DTK_R_SENTENCES = 8192
};
/* bits of evl_kind; at one cursor the calls fire in the order SEOT, TEOT, the Token ending there, SEPS */
enum { DTK_EVL_SEOT = 1, DTK_EVL_TEOT = 2, DTK_EVL_SEPS = 4 };
int dtk_batch_set_result_fields(dtk_batch *b, uint32_t fields);
int dtk_batch_download_begin(dtk_batch *b);
/* The HIP stream the result copies run on: the batch creates one with its first download; a caller with several
 * batches should lend them one stream between them (dtk_pipeline does): the HIP runtime maps streams onto four
 * hardware queues, and two streams on one queue serialise. */
int dtk_batch_set_download_stream(dtk_batch *b, void *hip_stream);
void *dtk_batch_download_stream(dtk_batch *b);
int dtk_batch_result_host(dtk_batch *b, dtk_result_view *out);

/* ---- a batch's sentences as rows: which tokens form a sentence, and its byte and rune span.
 *      The definition is a pure function of the reference's calls for one document (one TransduceTokenWriter call),
 *      scanned in order: a SENTENCE is a maximal non-empty run of Token calls with no SentenceEnd or TextEnd between
 *      them.  An open run is closed by a SentenceEnd, by a TextEnd, or by the end of the calls; a boundary with no
 *      token since the previous one makes no row.  Every token of a document belongs to exactly one sentence: row i
 *      of document d is the token range [sen_tok_end[i - 1], sen_tok_end[i]) of the document, with 0 in place of
 *      sen_tok_end[i - 1] at the document's first row.  This is the writer's own notion: a document has as many rows
 *      as the writer's Token closure pushes ints to sent[] (token_writer.go:75-79; sentB is true at the start and
 *      behind either kind of boundary), so rows(d) <= sent_off[d + 1] - sent_off[d] and dtk_totals.n_sent bounds n_sen.
 *        From the event bitmaps (every document not in exact_doc): f = 1 at the document's bit 0; then per cursor
 *      p = 0..len in ascending order, in the order the calls fire there: SEOT or TEOT set: f = 1; END set: that token
 *      is a sentence's first iff f, then f = 0; SEPS set: f = 1.  The tail word's calls come last and open nothing.
 *      The k-th END bit of a document is its k-th token: the first token of a row is the first k of the document's
 *      rows with tok_bend[k] >= cursor.  Documents in exact_doc get their rows from `calls` by the definition above;
 *      documents with a status bit get the rows this rule gives on what was delivered for them (a span whose token
 *      row does not exist reads as 0).
 *        dtk_batch_sentences_device: device pointers owned by the batch; the table is built on the batch's download
 *      stream and the call returns when it is complete.  dtk_batch_sentences_host: page-locked host memory; with
 *      DTK_R_SENTENCES among the result fields dtk_batch_download_begin has built and copied the table and the call
 *      only waits, without the bit it builds and copies on demand.  Both views are valid until the batch's next run
 *      or free.  Before a run, and after a run with DTK_NO_BYTE_OFFSETS: DTK_E_STATE (also, never expected, when a
 *      document in exact_doc has another number of Token calls than token rows).  (With documents in exact_doc
 *      the table is finished on the host and written back: a slow path that only crafted models reach.) ---- */
typedef struct {
  uint64_t n_sen;                  /* rows in the batch */
  const uint64_t *sen_off;         /* n_docs + 1: rows of document d are [sen_off[d], sen_off[d+1]) */
  const uint32_t *sen_tok_end;     /* document-relative: tokens of the document up to and including row i's last
                                      (the convention of text_tok_end) */
  const uint32_t *sen_bstart, *sen_bend;  /* tok_bstart of the row's first token, tok_bend of its last */
  const int32_t  *sen_rstart, *sen_rend;  /* tok_rstart of the first, tok_rend of the last (text-relative, so they
                                             follow DTK_NEWLINE_AFTER_EOT as the token rows do); NULL when the run
                                             had DTK_NO_RUNE_OFFSETS */
  const uint32_t *text_sen_end;    /* one per TextEnd, indexed like text_tok_end (text_off): rows of the document
                                      closed in front of that TextEnd (a TextEnd closes the open sentence first) */
} dtk_sentence_view;
int dtk_batch_sentences_device(dtk_batch *b, dtk_sentence_view *out);
int dtk_batch_sentences_host(dtk_batch *b, dtk_sentence_view *out);

/* ---- every token looked up in a vocabulary, on the device: type ids and a frequency list.
 *      A VOCABULARY is an ordered list of n_words byte strings (any bytes, empty ones too; at most 2^31 - 2 words and
 *      less than 2^32 bytes in all; of equal words the lowest index wins).  The KEY of a token is its surface as the
 *      reference's writer prints it, string(buf[offset:]) (token_writer.go:85,93): the document's bytes
 *      [tok_bstart, tok_bend) with every byte that does not decode (Go's DecodeRune: U+FFFD of width 1) replaced by
 *      EF BF BD -- what dtk_batch_render_* print, so a literal U+FFFD and an invalid byte give the same key.
 *      tok_id[i], in the batch-wide token order that tok_off indexes, is the index of the word equal to token i's key,
 *      or DTK_ID_UNKNOWN.  A row with tok_bstart > tok_bend (DTK_ST_BAD_OFFSET documents only) gets DTK_ID_UNKNOWN; the
 *      rows of a document with a status bit are looked up by the same rule on what was delivered for them, clamped to
 *      the document.  The result is exact: the table is hashed, but a match is decided by comparing the bytes.
 *        The object is built on the host and copied to the device of the calling thread (dtk_set_device); immutable
 *      afterwards and shareable between batches and threads, like a dtk_model.  Without a device dtk_vocab_create
 *      returns DTK_E_NO_DEVICE; offsets that do not ascend from 0 or exceed the limits are DTK_E_ARG.
 *      dtk_vocab_probe_mem needs no device: it builds the same table on the host and looks one key (the bytes after
 *      replacement) up with the code the kernel uses. ---- */
#define DTK_ID_UNKNOWN (-1)
typedef struct dtk_vocab dtk_vocab;
/* words: bytes[off[w] .. off[w+1]), off[0] == 0 */
int dtk_vocab_create(const uint8_t *bytes, const uint64_t *off, uint32_t n_words, dtk_vocab **out);
void dtk_vocab_free(dtk_vocab *v);
uint32_t dtk_vocab_size(const dtk_vocab *v);
int dtk_vocab_probe_mem(const uint8_t *bytes, const uint64_t *off, uint32_t n_words,
                        const uint8_t *key, size_t key_len, int32_t *id);
/* A tally: n_words + 1 64-bit counters on the vocabulary's device (the calling thread's must be that one, else
 * DTK_E_ARG), zero at creation.  Every run of a batch it is attached to adds that run's tokens exactly once -- 1 to the
 * counter of each token's id, unknown tokens to counter n_words -- when the run's lookup executes, however often the ids
 * are asked for or copied afterwards.  Integer adds: the counts are exact.  dtk_tally_read copies the counters to
 * counts[n_words + 1]: the sum over all lookups whose batch has been waited for -- an ids view was obtained,
 * dtk_batch_result_host returned, or the pipeline or stream run returned.  A frequency list needs nothing per token to
 * leave the device. */
typedef struct dtk_tally dtk_tally;
int dtk_tally_create(const dtk_vocab *v, dtk_tally **out);
int dtk_tally_read(dtk_tally *t, uint64_t *counts);
int dtk_tally_reset(dtk_tally *t);
void dtk_tally_free(dtk_tally *t);
/* v == NULL: off (the default; t must then be NULL too).  t may be NULL.  ids_home != 0: the ids are copied to
 * page-locked memory with the other result copies (dtk_batch_download_begin); 0: they stay in HBM until
 * dtk_batch_token_ids_host asks.  The vocabulary and the tally must outlive the batch's use of them and live on the
 * batch's device (else DTK_E_ARG, also for a tally of another vocabulary size).
 *   With a vocabulary attached dtk_batch_download_begin enqueues the lookup on the download stream, in front of the
 * copies; dtk_batch_token_ids_* begin it if nobody has, wait for it, and return device resp. page-locked host pointers,
 * valid until the batch's next run or free.  n_unknown counts the DTK_ID_UNKNOWN among the n_tok ids.  DTK_E_STATE before
 * a run, without a vocabulary, and after a run with DTK_NO_BYTE_OFFSETS.  No DTK_R_* bit belongs to the ids, and
 * dtk_result_view does not know them. */
int dtk_batch_set_vocab(dtk_batch *b, const dtk_vocab *v, dtk_tally *t, int ids_home);
typedef struct { uint64_t n_tok, n_unknown; const int32_t *tok_id; } dtk_token_id_view;
int dtk_batch_token_ids_device(dtk_batch *b, dtk_token_id_view *out);
int dtk_batch_token_ids_host(dtk_batch *b, dtk_token_id_view *out);

/* ---- every token split into WordPiece ids, on the device: what a BERT-style model takes.
 *      A SPLIT has four inputs: a dtk_vocab; a continuation PREFIX of 0..16 bytes ("##" for BERT vocabularies; empty is
 *      allowed); an unk_id with 0 <= unk_id < n_words; and max_runes, where 0 means 100, BERT's
 *      max_input_chars_per_word.  Anything outside these ranges is DTK_E_ARG.
 *        For token i the key K is exactly the key of dtk_batch_set_vocab above: the surface with every byte that does
 *      not decode replaced by EF BF BD, so K is valid UTF-8.  Then:
 *        - no key: a row with tok_bstart > tok_bend gives one piece, unk_id;
 *        - empty key: K empty gives zero pieces (BERT returns [] here);
 *        - too long: a key of more than max_runes runes gives one piece, unk_id;
 *        - otherwise, with start = 0, until start == len(K): take the largest end > start on a rune boundary of K such
 *          that a vocabulary word equals K[start:end) when start == 0, or prefix + K[start:end) otherwise (words are
 *          compared as bytes; of equal words the lowest index wins, as in dtk_vocab).  If there is no such end the whole
 *          token is the single piece unk_id (BERT's is_bad: no partial result, no backtracking).  Otherwise that word's
 *          index is the next piece and start = end.
 *      Without a fold (dtk_batch_set_fold below) the text is taken as it is.  With one, lower-casing and accent
 *      stripping -- what BERT's BasicTokenizer does in front of WordPiece -- happen where the key is read; CJK and
 *      punctuation splitting and whitespace cleaning stay with the caller.  A word that ends or begins inside a rune can
 *      never match, because cuts lie on rune boundaries only; neither can an empty word or the bare prefix.
 *        The outputs, in the batch-wide token order that tok_off indexes: piece_off[n_tok + 1], CSR; piece_id[n_pieces];
 *      piece_bend[n_pieces], the piece's end as a byte offset in its document, in SOURCE bytes (a replaced byte is one
 *      source byte and three key bytes): a piece begins at tok_bstart[i] or at its predecessor's end, and an unk_id piece
 *      for the whole token ends at tok_bend[i].  Rows of flagged documents are clamped to the document, as for the ids.
 *      n_unknown counts the tokens that became the single unk_id piece (no key, too long, or no such end).  The result
 *      is exact: the hash only picks where to look, the bytes decide.
 *        dtk_wordpiece_probe_mem needs no device: it builds the table on the host and splits one key -- the bytes after
 *      replacement, so `ends` are offsets in key bytes -- with the code the kernels use.  It stores up to `cap` pieces;
 *      with more it returns DTK_E_CAPACITY and *n_out is the needed count. ---- */
int dtk_wordpiece_probe_mem(const uint8_t *bytes, const uint64_t *off, uint32_t n_words,
                            const uint8_t *prefix, uint32_t prefix_len, int32_t unk_id, uint32_t max_runes,
                            const uint8_t *key, size_t key_len, int32_t *ids, uint32_t *ends, uint32_t cap, uint32_t *n_out);
/* v == NULL: off (the default).  pieces_home != 0: the pieces are copied to page-locked memory with the other result
 * copies (dtk_batch_download_begin); 0: they stay in HBM until dtk_batch_pieces_host asks.  The vocabulary must outlive
 * the batch's use of it and live on the batch's device (else DTK_E_ARG).  A vocabulary (dtk_batch_set_vocab) and a split
 * may be attached together, over the same dtk_vocab or different ones, and do not disturb each other.
 *   With a split attached dtk_batch_download_begin enqueues it on the download stream, in front of the copies, once per
 * run; dtk_batch_pieces_* begin it if nobody has and wait for it.  Which pointers a view holds is decided by the call
 * alone: dtk_batch_pieces_device always returns device pointers, also when pieces_home has brought a copy home beside
 * them, and dtk_batch_pieces_host always returns page-locked host pointers.  Both are valid until the batch's next run,
 * its next dtk_batch_set_wordpiece or its free.
 *   The output block is sized before the piece count is known, for half as many pieces again as tokens; a run with
 * more is split a second time when its pieces are asked for, and the batch's later runs start with a block of that
 * size.
 *   DTK_E_STATE before a run, without a split, and after a run with DTK_NO_BYTE_OFFSETS.  No DTK_R_* bit belongs to the
 * pieces, and dtk_result_view does not know them. */
int dtk_batch_set_wordpiece(dtk_batch *b, const dtk_vocab *v, const uint8_t *prefix, uint32_t prefix_len,
                            int32_t unk_id, uint32_t max_runes, int pieces_home);
typedef struct {
  uint64_t n_tok, n_pieces, n_unknown;
  const uint64_t *piece_off;
  const int32_t *piece_id;
  const uint32_t *piece_bend;
} dtk_piece_view;
int dtk_batch_pieces_device(dtk_batch *b, dtk_piece_view *out);
int dtk_batch_pieces_host(dtk_batch *b, dtk_piece_view *out);

/* ---- token keys folded on the device: uncased vocabularies and accent stripping, for the ids and the split above.
 *      A FOLD F is a finite map from a code point to a sequence of 0..DTK_FOLD_MAX (= 4) code points.  Code points not
 *      in the map fold to themselves.  Surrogates, values above U+10FFFF, duplicate sources and targets that are not
 *      scalar values are DTK_E_ARG, as are offsets that do not ascend from 0.  The map is data: the library embeds no
 *      Unicode tables.
 *        Let K be the key as defined above: the surface, with every undecodable byte as U+FFFD; K is valid UTF-8.  The
 *      FOLDED KEY is F(K): the UTF-8 of the folds of K's runes, in order; an invalid byte folds as U+FFFD.  Vocabulary
 *      words are NOT folded: the caller supplies a vocabulary that is already in folded form.
 *        Ids (dtk_batch_set_vocab) with a fold attached: tok_id[i] is the lowest index of the word equal to F(K), or
 *      DTK_ID_UNKNOWN.  An empty F(K) matches an empty word, as an empty key does without a fold.
 *        Split (dtk_batch_set_wordpiece) with a fold attached: the rule above stays, with these changes and nothing else:
 *        - cuts lie on rune boundaries of K, that is, on source runes;
 *        - the candidate for [start, end) is F(K[start:end)) when start == 0, or prefix + F(K[start:end)) otherwise;
 *        - a candidate whose fold is empty never matches, even if the vocabulary contains "" or the bare prefix;
 *        - "the largest end" is still taken: runes that fold to nothing behind a match therefore belong to that piece;
 *        - the last piece of a split token still ends at the clamped tok_bend;
 *        - max_runes counts the runes of F(K), which is what BERT's WordPiece sees;
 *        - a non-empty K with no such end is the single piece unk_id -- a token made only of stripped marks, or a
 *          remainder that folds to nothing with no preceding piece -- and counts in n_unknown;
 *        - piece_bend stays in SOURCE bytes, exactly as without a fold; no row gets zero pieces except an empty K;
 *        - the vocabulary's longest word bounds the FOLDED length of a candidate, never its source length.
 *      With no fold attached, every result is bit for bit what it is without this section.
 *        The object is built on the host and copied to the device of the calling thread; immutable afterwards and
 *      shareable between batches and threads, like a dtk_vocab.  Without a device dtk_fold_create returns
 *      DTK_E_NO_DEVICE.  dtk_fold_apply_mem needs no device: it writes F(K) of `key` -- any bytes, the undecodable ones
 *      as U+FFFD -- to out[cap]; *n_out is its length, and with more than cap bytes the call returns DTK_E_CAPACITY.
 *      dtk_wordpiece_probe_fold_mem is dtk_wordpiece_probe_mem under the fold given as arrays: `key` is K (valid UTF-8,
 *      else DTK_E_ARG) and `ends` are offsets in the bytes of the given key. ---- */
#define DTK_FOLD_MAX 4u
typedef struct dtk_fold dtk_fold;
/* source from[i] folds to to[to_off[i] .. to_off[i+1]); to_off[0] == 0 */
int dtk_fold_create(const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n, dtk_fold **out);
void dtk_fold_free(dtk_fold *f);
int dtk_fold_apply_mem(const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n,
                       const uint8_t *key, size_t key_len, uint8_t *out, size_t cap, size_t *n_out);
int dtk_wordpiece_probe_fold_mem(const uint8_t *bytes, const uint64_t *off, uint32_t n_words,
                                 const uint8_t *prefix, uint32_t prefix_len, int32_t unk_id, uint32_t max_runes,
                                 const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n,
                                 const uint8_t *key, size_t key_len, int32_t *ids, uint32_t *ends, uint32_t cap,
                                 uint32_t *n_out);
/* f == NULL: off (the default).  The fold applies to the batch's ids and to its split, must outlive the batch's use of
 * it and live on the batch's device (else DTK_E_ARG).  Setting or clearing it makes the finished run's ids, pieces and
 * model input rows stale: the next dtk_batch_token_ids_*, dtk_batch_pieces_* or dtk_batch_encoded_* call computes them
 * anew for that run (a tally attached to the ids then counts the run's tokens once more). */
int dtk_batch_set_fold(dtk_batch *b, const dtk_fold *f);

/* ---- sentences or documents as fixed-length model input rows, on the device: the matrix input_ids[n_rows x max_len]
 *      a BERT-style model takes, built behind the WordPiece split from what is resident in HBM.
 *      An ENCODING is a dtk_encode_spec: max_len, the row width, counted with the special positions; cls_id and sep_id,
 *      where a value >= 0 is written in front of / behind the body and -1 means that the position does not exist
 *      (n_special is the number of the two that exist); pad_id >= 0; unit; stride, the pieces consecutive windows of one
 *      unit share; flags.  With body = max_len - n_special and step = body - stride: body >= 1, 0 <= stride < body,
 *      max_len <= 65 535, unit one of the two values, no unknown flag, cls_id and sep_id >= -1, pad_id >= 0 -- anything
 *      else is DTK_E_ARG.
 *        UNITS.  DTK_ENC_SENTENCE: one unit per row of the sentence table (dtk_sentence_view above), in its batch-wide
 *      order; the unit's tokens are the row's [sen_tok_end[i - 1], sen_tok_end[i]) of its document, so a document without
 *      a token has no unit.  DTK_ENC_DOCUMENT: one unit per document, tokens [tok_off[d], tok_off[d + 1]); a document
 *      without a token is a unit of zero pieces.  A unit is a contiguous token range and therefore a contiguous range
 *      [P0, P0 + n) of piece_id.
 *        WINDOWS.  The unit makes w rows: w = 1 if n <= body or DTK_ENC_FIRST_WINDOW is set (plain truncation), else
 *      w = 1 + ceil((n - body) / step).  Window k holds the unit's pieces [k * step, min(k * step + body, n)).  Every unit
 *      makes at least one row; a unit without a piece makes the row of the specials alone.  (This is the rule of the
 *      `tokenizers` package's enable_truncation(max_length, stride): the first encoding followed by .overflowing.)
 *        ROWS.  Row r = unit_row_off[u] + k is window k of unit u: cls_id if it exists, the window's piece_ids, sep_id if
 *      it exists, pad_id up to max_len.
 *        The outputs: n_units, n_rows; n_cut, the units with n > body; max_len; unit_row_off[n_units + 1], CSR;
 *      input_ids[n_rows * max_len], row-major; row_len[n_rows], the positions in front of the padding, specials included
 *      (the attention mask is pos < row_len); row_piece0[n_rows], the batch-wide index into piece_id of the row's first
 *      body piece: position p of the body is piece row_piece0[r] + p - has_cls, from which piece_off gives the token and
 *      piece_bend the bytes; and with DTK_ENC_WORD_IDS word_id[n_rows * max_len], the document-relative index of the
 *      token the position's piece belongs to, -1 at specials and padding (NULL without the flag).  All of it is exact.
 *      Rows of documents with a status bit follow the same rule on whatever token rows and pieces were delivered.
 *        dtk_encode_rows_mem needs no device and runs the code the kernels run: a spec, piece_off[n_tok + 1], piece_id,
 *      the units as an ascending array of batch-wide token ends (unit u's tokens are [unit_tok_end[u - 1],
 *      unit_tok_end[u]), from 0), and -- only read with DTK_ENC_WORD_IDS -- tok_off[n_docs + 1].  It fills
 *      unit_row_off[n_units + 1] and, for up to cap_rows rows, the other arrays; *n_rows is the row count, and with
 *      cap_rows below it the call returns DTK_E_CAPACITY and no row array is complete.
 *        Out of scope: dtk_stream_* (a sentence can span a cut, and the pieces of the slice before it are gone),
 *      dtk_multi_*, pairs of sequences and token_type_ids, truncation and padding on the left. ---- */
enum { DTK_ENC_SENTENCE = 0, DTK_ENC_DOCUMENT = 1 };
enum { DTK_ENC_FIRST_WINDOW = 1, DTK_ENC_WORD_IDS = 2 };
typedef struct {
  uint32_t max_len;
  int32_t cls_id, sep_id, pad_id;
  uint32_t unit;     /* DTK_ENC_SENTENCE / DTK_ENC_DOCUMENT */
  uint32_t stride;
  uint32_t flags;    /* DTK_ENC_FIRST_WINDOW | DTK_ENC_WORD_IDS */
} dtk_encode_spec;
typedef struct {
  uint64_t n_units, n_rows, n_cut;
  uint32_t max_len;
  const uint64_t *unit_row_off;
  const int32_t *input_ids;
  const uint32_t *row_len;
  const uint64_t *row_piece0;
  const int32_t *word_id;
} dtk_encode_view;
int dtk_encode_rows_mem(const dtk_encode_spec *spec, const uint64_t *piece_off, uint64_t n_tok, const int32_t *piece_id,
                        const uint64_t *unit_tok_end, uint64_t n_units, const uint64_t *tok_off, uint32_t n_docs,
                        uint64_t cap_rows, uint64_t *unit_row_off, int32_t *input_ids, uint32_t *row_len,
                        uint64_t *row_piece0, int32_t *word_id, uint64_t *n_rows, uint64_t *n_cut);
/* spec == NULL: off (the default).  The stage runs behind the split of dtk_batch_set_wordpiece, which must be attached
 * too, on the download stream; for the sentence unit it builds the sentence table if nobody has.  rows_home has the
 * meaning of pieces_home: != 0 brings the rows to page-locked memory with the other result copies, 0 leaves them in HBM
 * until dtk_batch_encoded_host asks.  dtk_batch_download_begin enqueues the stage without waiting: the output block is
 * sized by n_rows <= n_units + n_pieces / step; a run whose split or whose sentence table had to be redone, or whose
 * rows exceed the block, wrote no row and is encoded again when its rows are asked for -- no view ever shows a partial
 * table.  (With documents in exact_doc the sentence table is finished on the host: the sentence unit then starts only
 * when its rows are asked for.)
 *   dtk_batch_encoded_device returns device pointers and dtk_batch_encoded_host page-locked host pointers, decided by
 * the call alone; both are valid until the batch's next run, its next dtk_batch_set_encode / dtk_batch_set_wordpiece or
 * its free.  A new spec or a new split makes a finished run be encoded anew when it is asked for.  DTK_E_STATE before a
 * run, without an encoding, without a split, and after a run with DTK_NO_BYTE_OFFSETS. */
int dtk_batch_set_encode(dtk_batch *b, const dtk_encode_spec *spec, int rows_home);
int dtk_batch_encoded_device(dtk_batch *b, dtk_encode_view *out);
int dtk_batch_encoded_host(dtk_batch *b, dtk_encode_view *out);

/* bit of position 0 of document d in the bitmaps of dtk_result_view.ev_bits */
#define DTK_EVENT_BIT(doc_off_d, d) (((uint64_t)(doc_off_d)) + (uint64_t)(d))

/* the bitmaps of dtk_result_view.ev_bits, in the order the calls fire at one cursor position (START is no call) */
enum {
  DTK_EVB_END = 0,   /* a token ends before this byte: Token(offset, buf) */
  DTK_EVB_START = 1, /* ... and this is its first byte */
  DTK_EVB_SEPS = 2,  /* SentenceEnd from an epsilon arc on an empty token (matrix.go:574-575), after an END here */
  DTK_EVB_TEOT = 3,  /* TextEnd fired by the EOT rune before this byte (matrix.go:599-600), before an END here */
  DTK_EVB_SEOT = 4,  /* SentenceEnd fired by that EOT rune (matrix.go:595-598), before its TextEnd */
  DTK_EVB_KINDS = 5
};
enum { DTK_TAIL_S = 1, DTK_TAIL_E = 2 }; /* doc_tail: final SentenceEnd (matrix.go:683-684) / TextEnd (:690-691) */

/* ---- NewTokenWriter(w, bits) (token_writer.go:36-175) for every document of the batch, rendered on
 *      the device: bytes[doc_off[d] .. doc_off[d+1]) is exactly what the reference writes to w for
 *      document d (surfaces + "\n", "\n" per sentence / text end, position lines) -- SIMPLE gives the
 *      stream of Transduce (matrix.go:340-342).  Call after dtk_batch_run; `bits` may differ from the
 *      run's flags except for DTK_NEWLINE_AFTER_EOT.  The view is owned by the batch (valid until the
 *      next run / render / free).  Documents flagged DTK_ST_EMPTY_TEXT make the reference panic in
 *      position modes; their bytes are unspecified. ---- */
typedef struct {
  const uint8_t *bytes;
  const uint64_t *doc_off; /* n_docs + 1 */
  uint64_t total;
} dtk_render_view;
int dtk_batch_render_device(dtk_batch *b, uint32_t bits, dtk_render_view *out);
int dtk_batch_render_host(dtk_batch *b, uint32_t bits, dtk_render_view *out);

/* ---- streaming: a corpus larger than one batch.  The reference streams any amount of input through a
 *      bufio.Reader (matrix.go:372); for many documents (one TransduceTokenWriter call each) the counterpart
 *      here is a pipeline of `depth` batches: the corpus is cut into slices of at most slice_bytes /
 *      slice_docs at document boundaries, slice i + 1 is uploaded (asynchronously, from page-locked host
 *      memory, on its batch's own HIP stream) while slice i is walked, and finished slices are handed to
 *      `fn` in order on the calling thread -- read their results there (dtk_batch_totals / result_* /
 *      render_*), they are valid until fn returns.  Text in memory from dtk_pinned_alloc is uploaded
 *      straight from there; other memory is page-locked for the duration of the call. ---- */
typedef struct dtk_pipeline dtk_pipeline;
typedef int (*dtk_slice_fn)(void *user, uint32_t first_doc, uint32_t n_docs, dtk_batch *slice); /* DTK_OK to go on */
int dtk_pipeline_create(uint64_t slice_bytes, uint32_t slice_docs, uint32_t depth, dtk_pipeline **out);
void dtk_pipeline_free(dtk_pipeline *p);
int dtk_pipeline_set_chunking(dtk_pipeline *p, uint32_t chunk_bytes, uint32_t warm_bytes);
/* fields != 0 (DTK_R_*): every slice's selected result arrays are brought to the host -- the copies of slice i start as
 * soon as its kernels have finished and run under the walk of slice i + 1 and the upload of slice i + 2; `fn` finds them
 * through dtk_batch_result_host.  0 (the default): results stay in HBM unless fn asks. */
int dtk_pipeline_set_result_fields(dtk_pipeline *p, uint32_t fields);
/* dtk_batch_set_vocab for every slice: `fn` finds a slice's ids through dtk_batch_token_ids_host (with result fields
 * selected and ids_home set, the ids of slice i come home under the walk of slice i + 1); every slice's lookup has been
 * waited for when `fn` gets the slice, so a tally holds the whole corpus when dtk_pipeline_run returns.  (dtk_multi_* has
 * no counterpart: a vocabulary lives on one device.) */
int dtk_pipeline_set_vocab(dtk_pipeline *p, const dtk_vocab *v, dtk_tally *t, int ids_home);
/* dtk_batch_set_wordpiece for every slice: `fn` finds a slice's pieces through dtk_batch_pieces_host; a slice is handed
 * over when its split has finished. */
int dtk_pipeline_set_wordpiece(dtk_pipeline *p, const dtk_vocab *v, const uint8_t *prefix, uint32_t prefix_len,
                               int32_t unk_id, uint32_t max_runes, int pieces_home);
/* dtk_batch_set_fold for every slice. */
int dtk_pipeline_set_fold(dtk_pipeline *p, const dtk_fold *f);
/* dtk_batch_set_encode for every slice: a slice is handed over when its encode has finished, and `fn` reads it through
 * dtk_batch_encoded_host.  Units and row_piece0 count from 0 in every slice, as piece_off does. */
int dtk_pipeline_set_encode(dtk_pipeline *p, const dtk_encode_spec *spec, int rows_home);
int dtk_pipeline_run(dtk_pipeline *p, const dtk_model *m, const uint8_t *text, const uint64_t *doc_off,
                     uint32_t n_docs, uint32_t flags, dtk_slice_fn fn, void *user);
/* ---- one stream of any length: the reference tokenizes whatever its reader delivers (bufio.Reader, matrix.go:373;
 *      cmd/datok.go:120-133 feeds a whole file or STDIN as ONE stream, texts separated by U+0004).  dtk_stream_run reads
 *      the stream through read_fn into page-locked buffers and walks it in slices of slice_bytes (S): slice k is the
 *      window [k * S, k * S + S + 8192) of the stream, walked as one document from the loop state its predecessor
 *      carried over, and ends at its cut -- the reference's first window rewind at or behind window byte S, proved exact
 *      like every lane start of the speculative walk.  Every call of the reference in front of the cut is the slice's;
 *      the calls from the cut on are the next slice's.  Host memory is depth * (S + 8192) bytes plus result buffers,
 *      whatever the stream's length.  The last slice ends where the stream does, with the final SentenceEnd / TextEnd.
 *        slice_fn gets the slices in order on the calling thread.  All positions of `view` (tok_bstart / tok_bend or the
 *      blocked form, evl_pos or the bitmaps, doc_tail) are relative to the window, whose byte 0 is stream byte `base`;
 *      a replay starts with the window start (buffer[0] of the reference) at `first`.  The writer's rune offsets and
 *      sentence list run across cuts (posC, sentB, init of token_writer.go:38-42): tok_rstart / tok_rend / sent of a
 *      slice's view -- the compaction's view of the window as a fresh document -- are not delivered, and
 *      dtk_stream_set_result_fields rejects the rune fields; the stream's offsets come as arrays of their own, 64-bit
 *      and computed on the device from the carried state (dtk_stream_set_offsets, dtk_stream_offsets), and its sentences
 *      as rows with the open row carried across the cuts (dtk_stream_set_sentences, dtk_stream_sentences).  The device renders a slice's writer bytes in every mode (`out` / `out_len`): in the four
 *      position-free modes (TOKENS, SENTENCES, both, neither; NEWLINE_AFTER_EOT changes nothing there) the writer is
 *      stateless (dtk_stream_set_render); with TOKEN_POS or SENTENCE_POS its state is carried from slice to slice on
 *      the device (dtk_stream_set_position_render, dtk_stream_emit).  A custom TokenWriter's closures are fed by the
 *      replay (include/datok.hpp, replay_list).
 *        *status: the OR of the slices' status bits; DTK_ST_EMPTY_TEXT is decided for the stream (a text may span cuts).
 *      A slice that needs the exact pass ends the run with DTK_E_IRREGULAR. ---- */
typedef struct dtk_stream dtk_stream;
typedef struct {
  uint64_t base;       /* stream offset of window byte 0 */
  uint32_t first;      /* window-relative: where this slice's calls begin (0 for the first slice, else the previous cut - S) */
  uint32_t cut;        /* window-relative: where they end; == len on the last slice */
  uint32_t len;        /* bytes of the window */
  uint32_t last;       /* 1: the stream's last slice -- view.doc_tail[0] holds the final SentenceEnd / TextEnd */
  uint32_t status;     /* the slice's DTK_ST_* bits, DTK_ST_EMPTY_TEXT decided with what the stream carried in */
  const uint8_t *text; /* the window's bytes (page-locked host memory), valid until slice_fn returns */
  dtk_result_view view;/* host pointers, one document; valid until slice_fn returns */
  const uint8_t *out;  /* dtk_stream_set_render: what NewTokenWriter(w, bits) writes for this slice's calls (page-locked */
  uint64_t out_len;    /* host memory, valid until slice_fn returns); NULL / 0 when rendering is off */
} dtk_stream_slice;
typedef size_t (*dtk_read_fn)(void *user, uint8_t *buf, size_t cap);       /* fills up to cap bytes; 0: end of the stream */
typedef int (*dtk_stream_slice_fn)(void *user, const dtk_stream_slice *s); /* DTK_OK to go on */
/* slice_bytes: a multiple of 256, at least 16 384 and below 2^31 (else DTK_E_ARG); depth: 2..16 buffers and batches
 * (3 and more: the read of slice k + 1 and the delivery of slice k - 1 run beside the walk of slice k). */
int dtk_stream_create(uint64_t slice_bytes, uint32_t depth, dtk_stream **out);
void dtk_stream_free(dtk_stream *s);
/* as dtk_batch_set_chunking; chunk_bytes 0 (one lane per slice), 16..2048 or 0xFFFFFFFF (by slice size) */
int dtk_stream_set_chunking(dtk_stream *s, uint32_t chunk_bytes, uint32_t warm_bytes);
/* The DTK_R_* arrays of every slice's view.  DTK_R_CSR, DTK_R_STATUS, DTK_R_TEXTS and DTK_R_EVENT_LIST always come;
 * the token bytes must be among them as DTK_R_TOK_BYTE or DTK_R_TOK_BYTE_BLK (else DTK_E_ARG).  Default: DTK_R_TOK_BYTE.
 * The rune fields (DTK_R_TOK_RUNE*, DTK_R_SENT) are DTK_E_ARG: a slice's view is the compaction's fresh-document view,
 * and the way to the stream's rune offsets and sentence list is dtk_stream_set_offsets.  DTK_R_SENTENCES is DTK_E_ARG
 * too: a sentence can span a cut, and the stream's rows come from dtk_stream_set_sentences, which carries the open one. */
int dtk_stream_set_result_fields(dtk_stream *s, uint32_t fields);
/* on != 0: every slice also brings the bytes a stock NewTokenWriter(w, bits) writes for its calls, rendered on the device
 * behind the slice's event list and in front of its copies (about one more byte per input byte on the link); the
 * slices' bytes one after the other are the stream's.  bits: DTK_TOKENS, DTK_SENTENCES, and DTK_NEWLINE_AFTER_EOT, which is
 * accepted and changes nothing; a position bit (their writer state runs across cuts) or an unknown bit: DTK_E_ARG.  The
 * view's arrays are delivered as before.  A token that the reference cannot print (DTK_ST_BAD_OFFSET) prints empty. */
int dtk_stream_set_render(dtk_stream *s, int on, uint32_t bits);
/* The same in the modes with a position bit: on != 0, every slice brings the bytes a stock NewTokenWriter(w, bits)
 * writes during its calls, rendered on the device from the writer's state behind its predecessor -- posC (64 bits: Go's
 * int), sentB, init, and whether pos / sent hold an integer -- which stays on the device between slices.
 * bits: any of the five writer bits with DTK_TOKEN_POS or DTK_SENTENCE_POS among them, else DTK_E_ARG; turning this
 * on turns dtk_stream_set_render off and the other way round.  dtk_stream_run must then get the same
 * DTK_NEWLINE_AFTER_EOT in its flags (else DTK_E_ARG).
 *   `out` / `out_len` of a slice are the writer's bytes in order, with two exceptions, both for a text that began in an
 * earlier slice or is still open at the cut (a position line is printed at TextEnd and holds a whole text's integers):
 *   - the position lines of a TextEnd whose text began in an earlier slice hold only the integers pushed in this
 *     slice, each behind a blank; what earlier slices pushed belongs at splice_pos / splice_sent;
 *   - the integers pushed in this slice for the text still open at the cut are not in `out`: they are the fragments
 *     open_pos / open_sent, blank-separated, with a blank in front if the line already has an integer.
 * dtk_stream_emit puts the two together.  A token whose end offset is 0 under DTK_NEWLINE_AFTER_EOT (the literal rule
 * of token_writer.go:51 would fire twice in one text) ends the run with DTK_E_IRREGULAR; more calls than the capacity
 * bound allows for, with DTK_E_CAPACITY.  Texts without a token (DTK_ST_EMPTY_TEXT; the reference panics) print as in
 * the C++ mirror: the SentenceEnd pushes nothing and an empty list prints no line. */
int dtk_stream_set_position_render(dtk_stream *s, int on, uint32_t bits);
typedef struct {
  int64_t posC;
  uint32_t sentB, init, pos_nonempty, sent_nonempty;
} dtk_stream_carry;
typedef struct {
  uint64_t splice_pos, splice_sent; /* offsets into out where the held TOKEN_POS / SENTENCE_POS prefix belongs; UINT64_MAX:
                                       none (at most one of each: only a slice's first text can be a continued one) */
  const uint8_t *open_pos;          /* the fragments of the text open at the cut (page-locked host memory, valid */
  uint64_t open_pos_len;            /* until slice_fn returns) */
  const uint8_t *open_sent;
  uint64_t open_sent_len;
  dtk_stream_carry carry_in, carry_out; /* the writer in front of and behind the slice */
} dtk_stream_pos;
/* Inside slice_fn, with position rendering on: the slice being delivered (else DTK_E_STATE). */
int dtk_stream_positions(dtk_stream *s, dtk_stream_pos *o);
typedef int (*dtk_write_fn)(void *user, const uint8_t *bytes, size_t n); /* DTK_OK to go on */
/* Inside slice_fn, once per slice: writes the slice's final bytes in order -- `out` with the held prefixes spliced in at
 * the two offsets -- and then appends the open fragments to the held prefixes.  Those live in the dtk_stream as host
 * strings, start empty with every run, and grow with the length of a TEXT (not of the stream), as the reference's pos[]
 * and sent[] do: some 11 bytes per token of the text that is open.  A non-zero return of w ends the call with it. */
int dtk_stream_emit(dtk_stream *s, dtk_write_fn w, void *user);
/* ---- a stream's rune offsets and sentence list as arrays: what the batch path hands out as tok_rstart / tok_rend /
 *      sent / text_tok_end / text_sent_end, for ONE stream of any length, slice by slice.
 * on != 0: every slice also brings the rune offsets and sentence list that a NewTokenWriter with
 * TOKEN_POS | SENTENCE_POS (and NEWLINE_AFTER_EOT iff dtk_stream_run's flags carry it) collects during the
 * slice's calls, computed on the device from the writer's state behind the predecessor, which stays on the device
 * between slices like position rendering's.  form: DTK_SO_PLAIN (16 B per token) or DTK_SO_BLOCKED (4.375), else
 * DTK_E_ARG.  May be on beside dtk_stream_set_render (the surfaces as text, the offsets as arrays) or alone; with
 * dtk_stream_set_position_render it is exclusive: turning either on while the other is on is DTK_E_ARG and changes
 * nothing.  dtk_stream_transduce turns it off.
 *   The slices' arrays one behind the other, the slice-relative text_tok_end / text_sent_end rebased by the running
 * counts of tokens and sent ints, are what one writer collects for the whole stream: the rows of a text that spans cuts
 * are the rows since the previous TextEnd, across slices.  Offsets are 64-bit: a stream without U+0004 is one text of any
 * length, and posC is Go's int.  A SentenceEnd in a text without a token pushes nothing (DTK_ST_EMPTY_TEXT; the
 * reference panics).  A token whose end offset is 0 under DTK_NEWLINE_AFTER_EOT ends the run with DTK_E_IRREGULAR, more
 * calls than the capacity bound allows for with DTK_E_CAPACITY, as in position rendering.
 *   The blocked form is dtk_off_block's, word for word, with 64-bit bases: tokens in the slice's order, block j holds
 * the tokens [64j, 64j + 64) of the slice, the last one is partial;
 *     brk   = the smallest lane l >= 1 of the block with start[64j + l] < end[64j + l - 1], or 64 if there is none
 *     base0 = the minimum over every start and end of the lanes < brk
 *     base1 = the minimum over the lanes >= brk, or 0 if brk == 64
 *     word[i] = (start[i] - base) | (end[i] - base) << 16   with base = lane < brk ? base0 : base1
 * A slice in which some segment of some block spans more than 65 535 gets the plain arrays in its place (copied when
 * the slice is delivered), and the blocked pointers are NULL. ---- */
enum { DTK_SO_PLAIN = 0, DTK_SO_BLOCKED = 1 };
int dtk_stream_set_offsets(dtk_stream *s, int on, uint32_t form);
typedef struct { int64_t base0, base1; uint32_t brk, reserved; } dtk_off_block64; /* 24 bytes */
DTK_BLK_DECODER int64_t dtk_blk64_start(const uint32_t *words, const dtk_off_block64 *heads, uint64_t i) {
  const dtk_off_block64 *h = heads + (i >> 6);
  return ((uint32_t)(i & 63u) < h->brk ? h->base0 : h->base1) + (int64_t)(words[i] & 0xFFFFu);
}
DTK_BLK_DECODER int64_t dtk_blk64_end(const uint32_t *words, const dtk_off_block64 *heads, uint64_t i) {
  const dtk_off_block64 *h = heads + (i >> 6);
  return ((uint32_t)(i & 63u) < h->brk ? h->base0 : h->base1) + (int64_t)(words[i] >> 16);
}
typedef struct {
  uint64_t n_tok, n_sent, n_text;          /* Token calls, ints pushed to sent[], TextEnd calls of THIS slice */
  const int64_t *tok_rstart, *tok_rend;    /* n_tok each; NULL when the blocked form was delivered */
  const uint32_t *tok_rblk;                /* n_tok words; NULL when the plain form was delivered */
  const dtk_off_block64 *tok_rblk_head;    /* ceil(n_tok / 64) */
  const int64_t *sent;                     /* n_sent, in push order */
  const uint32_t *text_tok_end, *text_sent_end; /* n_text each: tokens / sent ints of this slice in front of the g-th TextEnd */
  dtk_stream_carry carry_in, carry_out;    /* the writer in front of and behind the slice */
} dtk_stream_offs;
/* Inside slice_fn, with offset delivery on: the slice being delivered (else DTK_E_STATE).  Page-locked host memory,
 * valid until slice_fn returns. */
int dtk_stream_offsets(dtk_stream *s, dtk_stream_offs *o);
/* ---- a stream's sentences as rows: what the batch path hands out with DTK_R_SENTENCES (dtk_sentence_view), for ONE
 *      stream of any length, slice by slice.
 * The definition is the batch's, with the stream as one document: scan the reference's calls for the whole stream in
 * order; a sentence is a maximal non-empty run of Token calls with no SentenceEnd or TextEnd between them; a SentenceEnd,
 * a TextEnd or the end of the calls closes an open run; a boundary with no token since the previous one makes no row;
 * every token belongs to exactly one row.
 *   A row is delivered by the slice whose calls close it -- by a SentenceEnd or TextEnd call of that slice, on the last
 * slice also by the end of the calls behind the tail word's.  So every row arrives exactly once, complete and in order,
 * and the slices' rows one behind the other are the stream's table; a row whose tokens all lie in earlier slices still
 * arrives, with no token of the delivering slice (sen_tok_end 0).  What crosses a cut is the open row
 * (dtk_stream_sen_carry), chained on the device between slices like the writer's state; it starts as all-zero with
 * every run.
 *   on != 0: every slice also brings its rows, computed on the device behind the offsets chain of the slice (the rune
 * spans are the writer's offsets, as dtk_stream_offs delivers them, and DTK_NEWLINE_AFTER_EOT in dtk_stream_run's flags
 * moves them alike).  May be on alone -- then only the rows come home, some 36 B per sentence, and dtk_stream_offsets
 * answers DTK_E_STATE --, beside dtk_stream_set_offsets and beside dtk_stream_set_render; with
 * dtk_stream_set_position_render it is exclusive: turning either on while the other is on is DTK_E_ARG and changes
 * nothing.  dtk_stream_transduce turns it off.  DTK_E_IRREGULAR and DTK_E_CAPACITY end the run where offset delivery
 * gives them. ---- */
int dtk_stream_set_sentences(dtk_stream *s, int on);
typedef struct {
  uint32_t open, reserved;     /* a sentence is open at the cut (== !sentB of the writer's carry) */
  uint64_t bstart, bend;       /* stream byte offsets: start of its first token, end of its last so far */
  int64_t  rstart, rend;       /* the writer's rune offsets of the same two (text-relative, 64-bit like dtk_stream_offs) */
} dtk_stream_sen_carry;
typedef struct {
  uint64_t n_sen, n_text;                 /* rows closed by THIS slice's calls; TextEnd calls of this slice */
  const uint32_t *sen_tok_end;            /* tokens of THIS slice up to and including row i's last; 0 for a carried row that
                                             gets no token here; rebased by the running token count it is the stream's */
  const uint64_t *sen_bstart, *sen_bend;  /* stream byte offsets (slice base + window offset), first token's start / last token's end */
  const int64_t  *sen_rstart, *sen_rend;  /* tok_rstart of the first, tok_rend of the last, as dtk_stream_offs delivers them */
  const uint32_t *text_sen_end;           /* n_text: rows of THIS slice closed in front of the g-th TextEnd (a TextEnd closes the open row first) */
  dtk_stream_sen_carry carry_in, carry_out;
} dtk_stream_sens;
/* Inside slice_fn, with the sentence rows on: the slice being delivered (else DTK_E_STATE).  Page-locked host memory,
 * valid until slice_fn returns. */
int dtk_stream_sentences(dtk_stream *s, dtk_stream_sens *o);
/* ---- a stream's tokens looked up in a vocabulary (dtk_batch_set_vocab above), slice by slice.  A slice's batch is one
 *      document whose token rows are exactly the slice's Token calls, its bytes lie in the window, and a token never
 *      spans a cut: nothing is carried, every slice runs the batch's lookup behind its other outputs, and the slices' ids
 *      one behind the other are the ids of the stream as one document.  dtk_stream_token_ids, inside slice_fn: the slice
 *      being delivered (else DTK_E_STATE), page-locked host memory valid until slice_fn returns; with ids_home == 0 (a
 *      tally alone) tok_id is NULL and the counts are still there.  Every slice's lookup has been waited for when it is
 *      delivered.  dtk_stream_transduce leaves the vocabulary as set. ---- */
int dtk_stream_set_vocab(dtk_stream *s, const dtk_vocab *v, dtk_tally *t, int ids_home);
int dtk_stream_token_ids(dtk_stream *s, dtk_token_id_view *out);
/* ---- a stream's tokens split into WordPiece ids (dtk_batch_set_wordpiece above), slice by slice.  A token never spans
 *      a cut, so the slot's batch runs the batch's own split and nothing is carried: the slices' pieces one behind the
 *      other are the pieces of the stream as one document, except that piece_off counts from 0 in every slice and
 *      piece_bend is relative to the slice's window, as the slice's byte offsets are.  dtk_stream_pieces, inside
 *      slice_fn: the slice being delivered (else DTK_E_STATE), page-locked host memory valid until slice_fn returns; with
 *      pieces_home == 0 the three pointers are NULL and the counts are still there. ---- */
int dtk_stream_set_wordpiece(dtk_stream *s, const dtk_vocab *v, const uint8_t *prefix, uint32_t prefix_len,
                             int32_t unk_id, uint32_t max_runes, int pieces_home);
/* dtk_batch_set_fold for every slice of the stream. */
int dtk_stream_set_fold(dtk_stream *s, const dtk_fold *f);
int dtk_stream_pieces(dtk_stream *s, dtk_piece_view *out);
/* flags: DTK_NEWLINE_AFTER_EOT is accepted and changes nothing here (it only moves the writer's rune offsets), except
 * that with position rendering on it must be the bit dtk_stream_set_position_render got.  Short
 * reads are retried until a buffer is full; read_fn is not called again after it has returned 0. */
int dtk_stream_run(dtk_stream *s, const dtk_model *m, dtk_read_fn read_fn, void *read_user, uint32_t flags,
                   dtk_stream_slice_fn slice_fn, void *slice_user, uint32_t *status);
/* What the reference writes to w for the stream with a stock NewTokenWriter(w, bits), for a reader of any length.
 * Without a position bit the slices' rendered bytes are appended (dtk_stream_set_render is turned on with `bits`, and
 * stays so); with TOKEN_POS or SENTENCE_POS position rendering is turned on for the run, every slice's bytes come from
 * dtk_stream_emit, and both kinds of rendering are off afterwards.  *out is
 * malloc'd (the whole output: a caller that must bound that too writes from slice_fn, as `datok tokenize` does); free
 * with dtk_free. */
int dtk_stream_transduce(dtk_stream *s, const dtk_model *m, dtk_read_fn read_fn, void *read_user, uint32_t bits,
                         char **out, size_t *out_len, uint32_t *status);

/* ---- several GPUs of one node.  Documents are independent (matrix.go:349-381: all walk state is per call), so a corpus
 *      shards by slices with nothing to exchange: dtk_multi keeps one worker thread per listed device, each with its
 *      own replica of the model (loaded from model_path on that device) and its own dtk_pipeline; dtk_multi_run deals
 *      the slices of the corpus round-robin, every device works through its share, and finished slices are handed to
 *      `fn` on the calling thread in corpus order -- their results, if fields are selected, in the owning device's
 *      page-locked buffers (dtk_batch_result_host inside fn).  A device may be listed more than once.  This is the
 *      Go caller's multi-GPU entry point: fomafile.go:29-33 has no torch.distributed; the Python harness of bench.py
 *      (one process per GPU, RCCL gather) measures the same sharding from the other side. ---- */
typedef struct dtk_multi dtk_multi;
int dtk_multi_create(const char *model_path, const int *devices, uint32_t n_devices, uint64_t slice_bytes,
                     uint32_t slice_docs, uint32_t depth, dtk_multi **out);
void dtk_multi_free(dtk_multi *mp);
const char *dtk_multi_type(const dtk_multi *mp); /* Tokenizer.Type() */
int dtk_multi_set_result_fields(dtk_multi *mp, uint32_t fields);
int dtk_multi_set_chunking(dtk_multi *mp, uint32_t chunk_bytes, uint32_t warm_bytes);
int dtk_multi_run(dtk_multi *mp, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint32_t flags,
                  dtk_slice_fn fn, void *user);
void *dtk_pinned_alloc(size_t n); /* page-locked host memory (hipHostMalloc); NULL on failure */
void dtk_pinned_free(void *p);

/* ---- drop-in for Tokenizer.Transduce / TransduceTokenWriter with a stock
 *      NewTokenWriter(w, bits): what the reference writes to w for ONE stream
 *      (matrix.go:340-348, token_writer.go:36-175).  dtk_transduce walks and renders on the
 *      GPU; dtk_transduce_replay walks on the GPU and replays the event bytes into the
 *      closures of the C++ mirror of NewTokenWriter (include/datok.hpp) -- the path of a custom
 *      TokenWriter.  Both give the same bytes.  *out is malloc'd; free with
 *      dtk_free.  Returns 0 (the reference's `true`) or a negative code. ---- */
int dtk_transduce(const dtk_model *m, const uint8_t *text, size_t n, uint32_t bits,
                  char **out, size_t *out_len, uint32_t *status);
int dtk_transduce_replay(const dtk_model *m, const uint8_t *text, size_t n, uint32_t bits,
                         char **out, size_t *out_len, uint32_t *status);
/* Both keep one dtk_batch per calling thread between calls (sized for the largest input seen);
 * this frees the calling thread's. */
void dtk_transduce_release(void);
/* The walk of one stream on that per-thread batch: host pointers, valid until the thread's next
 * dtk_transduce* call -- what TransduceTokenWriter with a custom writer replays from. */
int dtk_transduce_result(const dtk_model *m, const uint8_t *text, size_t n, uint32_t flags, dtk_result_view *view);
void dtk_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
