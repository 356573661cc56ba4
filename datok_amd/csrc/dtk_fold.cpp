// dtk_fold.cpp -- the fold a batch's keys are read through (dtk_fold, include/datok_gpu.h).  The tables of
// dtk_fold_core.h are built on the host -- the ones the kernels and the host probe read through dtk_fold_rune -- and
// copied to the device; dtk_fold_apply_mem builds the same image and folds one key on the host, on a machine without a
// GPU too.
#include <algorithm>
#include <memory>
#include <vector>

#include "dtk_host.h"

int fold_image(const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n, FoldImage &img) {
  if (!to_off || to_off[0] != 0 || (n && !from)) return DTK_E_ARG;
  for (uint32_t i = 0; i < n; i++) {
    if (to_off[i + 1] < to_off[i] || to_off[i + 1] - to_off[i] > DTK_FOLD_MAX || !dtk_fold_scalar(from[i])) return DTK_E_ARG;
    if (to_off[i + 1] >= 0x10000000u) return DTK_E_ARG;  // (an entry has 28 bits for an offset)
  }
  if (to_off[n] && !to) return DTK_E_ARG;
  for (uint32_t k = 0; k < to_off[n]; k++)
    if (!dtk_fold_scalar(to[k])) return DTK_E_ARG;
  try {
    std::vector<uint32_t> sorted(from, from + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return DTK_E_ARG;
    // a block per page with a source, in ascending page order behind the ASCII page's
    std::vector<uint16_t> page(DTK_FOLD_PAGES, 0);
    uint32_t blocks = 1;
    for (uint32_t cp : sorted) {
      const uint32_t pg = cp / DTK_FOLD_PAGE;
      if (pg && !page[pg]) page[pg] = (uint16_t)blocks++;
    }
    std::vector<uint32_t> multi;
    img.words.assign((size_t)blocks * DTK_FOLD_PAGE, 0u);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t cp = from[i], cnt = to_off[i + 1] - to_off[i];
      uint32_t e;
      if (cnt == 1u) {
        e = dtk_fold_entry_of(1u, to[to_off[i]]);
      } else {
        e = dtk_fold_entry_of(cnt, (uint32_t)multi.size());
        multi.insert(multi.end(), to + to_off[i], to + to_off[i + 1]);
      }
      img.words[(size_t)page[cp / DTK_FOLD_PAGE] * DTK_FOLD_PAGE + cp % DTK_FOLD_PAGE] = e;
    }
    img.multi_at = img.words.size();
    img.words.insert(img.words.end(), multi.begin(), multi.end());
    img.page_at = img.words.size();
    img.words.resize(img.page_at + DTK_FOLD_PAGES / 2, 0u);
    std::copy(page.begin(), page.end(), reinterpret_cast<uint16_t *>(img.words.data() + img.page_at));
  } catch (const std::bad_alloc &) {
    return DTK_E_NOMEM;
  }
  return DTK_OK;
}

extern "C" int dtk_fold_apply_mem(const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n,
                                  const uint8_t *key, size_t key_len, uint8_t *out, size_t cap, size_t *n_out) {
  if (!n_out || (key_len && !key) || key_len >= (1ull << 32) || (cap && !out)) return DTK_E_ARG;
  FoldImage img;
  const int rc = fold_image(from, to_off, to, n, img);
  if (rc != DTK_OK) return rc;
  const DtkFoldDev F = img.view(img.words.data());
  // K's runes the way Go ranges over the bytes: one that does not decode is U+FFFD of width 1
  size_t k = 0;
  const uint32_t len = (uint32_t)key_len;
  for (uint32_t i = 0; i < len;) {
    const uint32_t c = key[i];
    uint32_t cp = c, width = 1;
    if (c >= 0xC0u) {
      cp = dtk_utf8_lead([&](uint32_t j) { return (uint32_t)key[j]; }, i, len, c);
      if (cp != 0xFFFDu) width = cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u;
      else if (len - i >= 3u && c == 0xEFu && key[i + 1] == 0xBFu && key[i + 2] == 0xBDu) width = 3u;  // U+FFFD itself
    } else if (c >= 0x80u) {
      cp = 0xFFFDu;  // a continuation byte no rune owns
    }
    i += width;
    uint32_t t[DTK_FOLD_MAX];
    const uint32_t m = dtk_fold_rune(F, cp, t);
    for (uint32_t j = 0; j < m; j++)
      dtk_utf8_put(t[j], [&](uint32_t b) { if (k < cap) out[k] = (uint8_t)b; k++; });
  }
  *n_out = k;
  return k > cap ? DTK_E_CAPACITY : DTK_OK;
}

extern "C" int dtk_fold_create(const uint32_t *from, const uint32_t *to_off, const uint32_t *to, uint32_t n, dtk_fold **out) {
  if (!out) return DTK_E_ARG;
  *out = nullptr;
  FoldImage img;
  int rc = fold_image(from, to_off, to, n, img);
  if (rc != DTK_OK) return rc;
  if (dtk_device_count() <= 0) return DTK_E_NO_DEVICE;
  std::unique_ptr<dtk_fold> f(new dtk_fold());
  HIP_TRY(hipGetDevice(&f->device));
  const uint64_t words = img.words.size();
  if ((rc = f->d_words.fit(words, words)) != DTK_OK) return rc;
  HIP_TRY(hipMemcpy(f->d_words.p, img.words.data(), words * 4, hipMemcpyHostToDevice));
  f->dev = img.view(f->d_words.p);
  *out = f.release();
  return DTK_OK;
}

extern "C" void dtk_fold_free(dtk_fold *f) { delete f; }
