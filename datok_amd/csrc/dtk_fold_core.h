// dtk_fold_core.h -- a fold's one definition (include/datok_gpu.h, dtk_fold_create), for the host and for gfx950: a finite
// map from a code point to 0..DTK_FOLD_MAX code points, applied rune by rune to a token's key where the key is read
// (dtk_wordpiece_core.h: DtkFoldedKey).  dtk_fold_apply_mem and the host probe (dtk_fold.cpp, dtk_vocab.cpp) and the
// kernels of dtk_tokenid.hip and dtk_wordpiece.hip all go through dtk_fold_rune, so they cannot drift apart.  The map is
// data: nothing here knows a Unicode table.
//
// The table: blocks of DTK_FOLD_PAGE 32-bit entries.  page[cp >> 7] is the block of cp's page, 0 for a page without a
// source -- except for page 0 itself, the ASCII page, whose block is block 0 and always there: the kernels stage it in
// LDS, so an ASCII byte costs no global load.  An entry is
//   0                            cp folds to itself
//   t + 1  (bit 31 clear)        cp folds to the one code point t
//   bit 31, n << 28, o           cp folds to the n code points multi[o .. o + n), n = 0 or 2..DTK_FOLD_MAX
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define DTK_VH __host__ __device__ __forceinline__
#else
#define DTK_VH inline
#endif

#define DTK_FOLD_MAX 4u          // the code points one source folds to, at most
#define DTK_FOLD_PAGE 128u       // the code points of a page
#define DTK_FOLD_PAGES 8704u     // 0x110000 / DTK_FOLD_PAGE
#define DTK_FOLD_MULTI 0x80000000u
#define DTK_FOLD_MAX_BYTES 16u   // DTK_FOLD_MAX code points of 4 bytes: the key bytes of one source rune, at most

struct DtkFoldDev {
  const uint32_t *entry;  // blocks * DTK_FOLD_PAGE; block 0: the ASCII page.  Null: no fold
  const uint16_t *page;   // DTK_FOLD_PAGES
  const uint32_t *multi;
};

DTK_VH bool dtk_fold_scalar(uint32_t cp) { return cp <= 0x10FFFFu && (cp < 0xD800u || cp > 0xDFFFu); }

DTK_VH uint32_t dtk_fold_entry_of(uint32_t n, uint32_t first_or_offset) {
  return n == 1u ? first_or_offset + 1u : DTK_FOLD_MULTI | (n << 28) | first_or_offset;
}

// cp's entry; ascii: block 0, wherever the caller keeps it
DTK_VH uint32_t dtk_fold_entry(const DtkFoldDev &F, const uint32_t *ascii, uint32_t cp) {
  if (cp < DTK_FOLD_PAGE) return ascii[cp];
  if (cp > 0x10FFFFu) return 0u;
  const uint32_t b = F.page[cp / DTK_FOLD_PAGE];
  return b ? F.entry[b * DTK_FOLD_PAGE + cp % DTK_FOLD_PAGE] : 0u;
}

// what entry e of cp says: the code points into out, their number returned
DTK_VH uint32_t dtk_fold_expand(const DtkFoldDev &F, uint32_t e, uint32_t cp, uint32_t out[DTK_FOLD_MAX]) {
  if (e == 0u) { out[0] = cp; return 1u; }
  if (!(e & DTK_FOLD_MULTI)) { out[0] = e - 1u; return 1u; }
  const uint32_t n = (e >> 28) & 7u, o = e & 0x0FFFFFFFu;
  for (uint32_t k = 0; k < n && k < DTK_FOLD_MAX; k++) out[k] = F.multi[o + k];
  return n < DTK_FOLD_MAX ? n : DTK_FOLD_MAX;
}

// F(cp): the code points cp folds to, 0..DTK_FOLD_MAX of them
DTK_VH uint32_t dtk_fold_rune(const DtkFoldDev &F, uint32_t cp, uint32_t out[DTK_FOLD_MAX]) {
  return dtk_fold_expand(F, dtk_fold_entry(F, F.entry, cp), cp, out);
}

// The UTF-8 of scalar value cp, byte by byte into put(byte).
template <class Put>
DTK_VH void dtk_utf8_put(uint32_t cp, Put put) {
  if (cp < 0x80u) {
    put(cp);
  } else if (cp < 0x800u) {
    put(0xC0u | (cp >> 6)); put(0x80u | (cp & 0x3Fu));
  } else if (cp < 0x10000u) {
    put(0xE0u | (cp >> 12)); put(0x80u | ((cp >> 6) & 0x3Fu)); put(0x80u | (cp & 0x3Fu));
  } else {
    put(0xF0u | (cp >> 18)); put(0x80u | ((cp >> 12) & 0x3Fu)); put(0x80u | ((cp >> 6) & 0x3Fu)); put(0x80u | (cp & 0x3Fu));
  }
}

// The rune that begins at position i of `n` bytes read through at(j) (a byte; anything else ends a sequence), c = at(i)
// >= 0xC0: the way Go decodes it -- shortest form, no surrogate, at most U+10FFFF -- or U+FFFD where none decodes.
// Nothing at or behind n is read.
template <class At>
DTK_VH uint32_t dtk_utf8_lead(At at, uint32_t i, uint32_t n, uint32_t c) {
  const uint32_t more = c >= 0xF0u ? 3u : c >= 0xE0u ? 2u : 1u;
  if (c >= 0xF8u || n - i <= more) return 0xFFFDu;
  uint32_t cp = c & (0x3Fu >> more);
  for (uint32_t k = 1; k <= more; k++) {
    const uint32_t b = at(i + k);
    if ((b & ~0x3Fu) != 0x80u) return 0xFFFDu;
    cp = (cp << 6) | (b & 0x3Fu);
  }
  const uint32_t least = more == 1u ? 0x80u : more == 2u ? 0x800u : 0x10000u;
  return cp >= least && dtk_fold_scalar(cp) ? cp : 0xFFFDu;
}
