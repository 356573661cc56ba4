// dtk_encode_core.h -- the encoding rule's one definition (include/datok_gpu.h, dtk_batch_set_encode), for the host and
// for gfx950: dtk_encode_rows_mem (dtk_encode.cpp) and the kernels of dtk_encode.hip call the functions below, so they
// cannot drift apart.  A unit is a contiguous token range [t0, t1) of the batch, hence a contiguous range of piece_id:
// n = piece_off[t1] - piece_off[t0] pieces from P0 = piece_off[t0] on.
//   dtk_enc_rule      the validity of a spec, and the numbers every other function needs
//   dtk_enc_windows   the rows a unit of n pieces makes
//   dtk_enc_window    the pieces of window k, relative to the unit
//   dtk_enc_value     what stands at position p of a row
//   dtk_enc_token     the token a body piece belongs to: an upper bound in piece_off over the unit's token range
#pragma once
#include <stdint.h>

#include "dtk_vocab_core.h"  // DTK_VH

// the header's values (include/datok_gpu.h; dtk_encode.cpp checks that they are): the kernel units do not see it
#define DTK_ENCK_SENTENCE 0u
#define DTK_ENCK_DOCUMENT 1u
#define DTK_ENCK_FIRST_WINDOW 1u
#define DTK_ENCK_WORD_IDS 2u
// a dtk_encode_spec, field by field
struct DtkEncSpec {
  uint32_t max_len;
  int32_t cls_id, sep_id, pad_id;
  uint32_t unit, stride, flags;
};

struct DtkEncRule {
  uint32_t max_len, body, step;   // body = max_len - n_special, step = body - stride
  uint32_t has_cls, has_sep;      // 0 or 1
  int32_t cls_id, sep_id, pad_id;
  uint32_t unit, flags;
};

// false: the spec is none (DTK_E_ARG)
DTK_VH bool dtk_enc_rule(const DtkEncSpec &s, DtkEncRule &r) {
  r = DtkEncRule{};
  if (s.cls_id < -1 || s.sep_id < -1 || s.pad_id < 0) return false;
  if (s.unit != DTK_ENCK_SENTENCE && s.unit != DTK_ENCK_DOCUMENT) return false;
  if (s.flags & ~(uint32_t)(DTK_ENCK_FIRST_WINDOW | DTK_ENCK_WORD_IDS)) return false;
  const uint32_t has_cls = s.cls_id >= 0 ? 1u : 0u, has_sep = s.sep_id >= 0 ? 1u : 0u;
  if (s.max_len > 65535u || s.max_len < has_cls + has_sep + 1u) return false;  // (body >= 1)
  const uint32_t body = s.max_len - has_cls - has_sep;
  if (s.stride >= body) return false;
  r.max_len = s.max_len; r.body = body; r.step = body - s.stride;
  r.has_cls = has_cls; r.has_sep = has_sep;
  r.cls_id = s.cls_id; r.sep_id = s.sep_id; r.pad_id = s.pad_id;
  r.unit = s.unit; r.flags = s.flags;
  return true;
}

// the rows of a unit of n pieces: at least one
DTK_VH uint64_t dtk_enc_windows(const DtkEncRule &r, uint64_t n) {
  if (n <= r.body || (r.flags & DTK_ENCK_FIRST_WINDOW)) return 1u;
  return 1u + (n - r.body + r.step - 1u) / r.step;
}

// window k of a unit of n pieces holds the unit's pieces [first, first + len)
DTK_VH void dtk_enc_window(const DtkEncRule &r, uint64_t n, uint64_t k, uint64_t &first, uint32_t &len) {
  first = k * r.step;
  const uint64_t end = first + r.body < n ? first + r.body : n;
  len = (uint32_t)(end > first ? end - first : 0u);
}

// positions in front of the padding
DTK_VH uint32_t dtk_enc_row_len(const DtkEncRule &r, uint32_t len) { return r.has_cls + len + r.has_sep; }

// position p of a row is a piece of the body
DTK_VH bool dtk_enc_in_body(const DtkEncRule &r, uint32_t len, uint32_t p) { return p >= r.has_cls && p - r.has_cls < len; }

// the id at position p of a row whose window of len pieces begins at win[0]
DTK_VH int32_t dtk_enc_value(const DtkEncRule &r, uint32_t len, uint32_t p, const int32_t *win) {
  if (p < r.has_cls) return r.cls_id;
  const uint32_t q = p - r.has_cls;
  if (q < len) return win[q];
  return q == len && r.has_sep ? r.sep_id : r.pad_id;
}

// The token of piece q (batch-wide) of a unit with tokens [t0, t1), t0 < t1 and piece_off[t0] <= q < piece_off[t1]: the
// last t with piece_off[t] <= q -- a token without a piece shares its offset with its successor and is passed over.
DTK_VH uint64_t dtk_enc_token(const uint64_t *piece_off, uint64_t t0, uint64_t t1, uint64_t q) {
  uint64_t lo = t0, hi = t1;
  while (hi - lo > 1u) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (piece_off[mid] <= q) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- the kernels' arguments (dtk_encode.hip)
#define DTK_ENC_TILE 256u  // units of one block round: a scan tile
// what the count leaves per unit for the write
struct DtkEncUnit {
  uint64_t row_loc;  // the unit's first row, counted inside its tile
  uint64_t p0, n;    // its pieces: piece_id[p0 .. p0 + n)
  uint64_t t0, t1;   // its tokens, batch-wide
  uint64_t tok0;     // tok_off of its document
};
struct DtkEncodeArgs {
  struct DtkEncRule rule;
  const uint64_t *tok_off;       // n_docs + 1
  uint32_t n_docs;
  uint64_t n_tok;
  // DTK_ENCK_SENTENCE: the sentence table and its count word; with more rows than sen_cap the table was not written
  const uint64_t *sen_off;       // n_docs + 1
  const uint32_t *sen_tok_end;
  const uint32_t *sen_count;
  uint64_t sen_cap;
  const uint64_t *piece_off;     // n_tok + 1 (always written by the split)
  const int32_t *piece_id;       // written only if piece_off[n_tok] <= piece_cap
  uint64_t piece_cap;
  uint64_t units_cap, rows_cap;  // what the workspace and the outputs hold
  struct DtkEncUnit *unit;       // workspace, units_cap
  uint64_t *tile_base;           // workspace, tiles + 1: a tile's rows, then their exclusive scan and the total
  unsigned long long *cnt;       // device words [n_rows, n_cut, n_units, ok]; n_cut cleared in front of the launch
  uint64_t *unit_row_off;        // units_cap + 1
  int32_t *input_ids;            // rows_cap * max_len, 16-byte aligned
  uint32_t *row_len;             // rows_cap
  uint64_t *row_piece0;          // rows_cap
  int32_t *word_id;              // rows_cap * max_len, 16-byte aligned, or null
};
DTK_VH uint64_t dtk_enc_tiles(uint64_t n_units) { return (n_units + DTK_ENC_TILE - 1u) / DTK_ENC_TILE; }
extern "C" int dtk_launch_encode(const DtkEncodeArgs *args, void *stream);
