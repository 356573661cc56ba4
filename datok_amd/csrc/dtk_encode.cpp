// dtk_encode.cpp -- dtk_encode_rows_mem: the encoding rule of dtk_encode_core.h applied on the host, without a device
// (include/datok_gpu.h).  What the kernels of dtk_encode.hip compute, from the same functions; the unit's token range
// is the caller's here and the sentence table's or tok_off's there.
#include <algorithm>

#include "dtk_host.h"

static_assert(DTK_ENC_SENTENCE == DTK_ENCK_SENTENCE && DTK_ENC_DOCUMENT == DTK_ENCK_DOCUMENT &&
                  DTK_ENC_FIRST_WINDOW == DTK_ENCK_FIRST_WINDOW && DTK_ENC_WORD_IDS == DTK_ENCK_WORD_IDS,
              "the rule's values are the header's");

bool enc_rule_of(const dtk_encode_spec *s, DtkEncRule *r) {
  return s && dtk_enc_rule(DtkEncSpec{s->max_len, s->cls_id, s->sep_id, s->pad_id, s->unit, s->stride, s->flags}, *r);
}

extern "C" int dtk_encode_rows_mem(const dtk_encode_spec *spec, const uint64_t *piece_off, uint64_t n_tok,
                                   const int32_t *piece_id, const uint64_t *unit_tok_end, uint64_t n_units,
                                   const uint64_t *tok_off, uint32_t n_docs, uint64_t cap_rows, uint64_t *unit_row_off,
                                   int32_t *input_ids, uint32_t *row_len, uint64_t *row_piece0, int32_t *word_id,
                                   uint64_t *n_rows, uint64_t *n_cut) {
  DtkEncRule R;
  if (!enc_rule_of(spec, &R) || !piece_off || !n_rows || !unit_row_off || (n_units && !unit_tok_end)) return DTK_E_ARG;
  const bool words = (R.flags & DTK_ENC_WORD_IDS) != 0;
  if (cap_rows && (!input_ids || !row_len || !row_piece0 || (words && !word_id))) return DTK_E_ARG;
  if (words && (!tok_off || !n_docs || tok_off[0] != 0 || tok_off[n_docs] != n_tok)) return DTK_E_ARG;
  for (uint64_t t = 0; t < n_tok; t++)
    if (piece_off[t + 1] < piece_off[t]) return DTK_E_ARG;
  if (piece_off[n_tok] && !piece_id) return DTK_E_ARG;
  for (uint64_t u = 0; u < n_units; u++)
    if (unit_tok_end[u] > n_tok || (u && unit_tok_end[u] < unit_tok_end[u - 1])) return DTK_E_ARG;
  if (words)
    for (uint32_t d = 0; d < n_docs; d++)
      if (tok_off[d + 1] < tok_off[d]) return DTK_E_ARG;
  uint64_t rows = 0, cut = 0;
  for (uint64_t u = 0; u < n_units; u++) {
    const uint64_t t0 = u ? unit_tok_end[u - 1] : 0u, t1 = unit_tok_end[u];
    const uint64_t p0 = piece_off[t0], n = piece_off[t1] - p0;
    // the unit's document: the last d with tok_off[d] <= t0 (a unit of no token has no body position to ask)
    const uint64_t tok0 = words && t0 < t1 ? *(std::upper_bound(tok_off, tok_off + n_docs, t0) - 1) : 0u;
    unit_row_off[u] = rows;
    cut += n > R.body ? 1u : 0u;
    const uint64_t w = dtk_enc_windows(R, n);
    for (uint64_t k = 0; k < w; k++) {
      const uint64_t r = rows + k;
      if (r >= cap_rows) continue;  // (counted, not stored)
      uint64_t first;
      uint32_t len;
      dtk_enc_window(R, n, k, first, len);
      row_len[r] = dtk_enc_row_len(R, len);
      row_piece0[r] = p0 + first;
      const int32_t *win = len ? piece_id + p0 + first : nullptr;
      for (uint32_t p = 0; p < R.max_len; p++) {
        input_ids[r * R.max_len + p] = dtk_enc_value(R, len, p, win);
        if (words)
          word_id[r * R.max_len + p] =
              dtk_enc_in_body(R, len, p) ? (int32_t)(dtk_enc_token(piece_off, t0, t1, p0 + first + (p - R.has_cls)) - tok0) : -1;
      }
    }
    rows += w;
  }
  unit_row_off[n_units] = rows;
  *n_rows = rows;
  if (n_cut) *n_cut = cut;
  return rows > cap_rows ? DTK_E_CAPACITY : DTK_OK;
}
