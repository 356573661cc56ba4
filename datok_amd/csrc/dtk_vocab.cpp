// dtk_vocab.cpp -- the vocabulary a run's tokens are looked up in (dtk_vocab, include/datok_gpu.h) and the counters of
// a frequency list (dtk_tally).  The table is built on the host with the functions of dtk_vocab_core.h -- the ones the
// lookup kernel (dtk_tokenid.hip) probes it with -- and copied to the device; dtk_vocab_probe_mem builds the same image
// and probes it on the host, on a machine without a GPU too.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "dtk_host.h"

namespace {
// The table on the host.  `view` reads the caller's bytes in place.
struct VocabImage {
  std::vector<uint64_t> slots;
  std::vector<uint32_t> off;
  DtkVocabDev view{};
};

uint64_t hash_key(const uint8_t *key, size_t n, int32_t hash_bits) {
  DtkVocabHash h = dtk_vh_init();
  for (size_t i = 0; i < n; i++) dtk_vh_byte(h, key[i]);
  return dtk_vh_finish(h, n, hash_bits);
}

int32_t find_key(const DtkVocabDev &V, const uint8_t *key, size_t n, uint32_t *free_slot) {
  return dtk_vocab_find(
      V, hash_key(key, n, V.hash_bits),
      [&](uint32_t w) { return V.off[w + 1] - V.off[w] == n && (n == 0 || memcmp(V.bytes + V.off[w], key, n) == 0); },
      free_slot);
}

int build_image(const uint8_t *bytes, const uint64_t *off, uint32_t n_words, VocabImage &img) {
  if (!off || off[0] != 0 || n_words > 0x7FFFFFFEu) return DTK_E_ARG;
  for (uint32_t w = 0; w < n_words; w++)
    if (off[w + 1] < off[w] || off[w + 1] >= (1ull << 32)) return DTK_E_ARG;
  if (off[n_words] && !bytes) return DTK_E_ARG;
  uint64_t n_slots = 2;
  while (n_slots < 2 * (uint64_t)n_words) n_slots *= 2;
  try {
    img.slots.assign((size_t)n_slots, 0);
    img.off.resize((size_t)n_words + 1);
  } catch (const std::bad_alloc &) {
    return DTK_E_NOMEM;
  }
  for (uint32_t w = 0; w <= n_words; w++) img.off[w] = (uint32_t)off[w];
  img.view = DtkVocabDev{img.slots.data(), img.off.data(), bytes, (uint32_t)(n_slots - 1), n_words, g_dbg.vocab_hash_bits,
                         vocab_max_word(off, n_words)};
  // in ascending order, and a word that is there already is left out: of equal words the lowest index wins
  for (uint32_t w = 0; w < n_words; w++) {
    const uint8_t *key = bytes + off[w];
    const size_t n = (size_t)(off[w + 1] - off[w]);
    uint32_t slot = 0;
    if (find_key(img.view, key, n, &slot) < 0) img.slots[slot] = dtk_vh_entry(hash_key(key, n, img.view.hash_bits), w);
  }
  return DTK_OK;
}
}  // namespace

uint32_t vocab_max_word(const uint64_t *off, uint32_t n_words) {
  uint64_t m = 0;
  for (uint32_t w = 0; w < n_words; w++) m = std::max(m, off[w + 1] - off[w]);
  return (uint32_t)m;  // (build_image has checked that every offset is below 2^32)
}

// The arguments of a split, as dtk_batch_set_wordpiece and dtk_wordpiece_probe_mem take them.
int wordpiece_rule(uint32_t n_words, const uint8_t *prefix, uint32_t prefix_len, int32_t unk_id, uint32_t max_runes,
                   DtkWpRule *rule) {
  if (prefix_len > DTK_WP_MAX_PREFIX || (prefix_len && !prefix) || unk_id < 0 || (uint32_t)unk_id >= n_words) return DTK_E_ARG;
  *rule = dtk_wp_rule(prefix, prefix_len, unk_id, max_runes);
  return DTK_OK;
}

extern "C" int dtk_wordpiece_probe_mem(const uint8_t *bytes, const uint64_t *off, uint32_t n_words, const uint8_t *prefix,
                                       uint32_t prefix_len, int32_t unk_id, uint32_t max_runes, const uint8_t *key,
                                       size_t key_len, int32_t *ids, uint32_t *ends, uint32_t cap, uint32_t *n_out) {
  if (!n_out || (key_len && !key) || key_len >= (1ull << 32) || (cap && (!ids || !ends))) return DTK_E_ARG;
  VocabImage img;
  DtkWpRule rule;
  int rc = build_image(bytes, off, n_words, img);
  if (rc != DTK_OK || (rc = wordpiece_rule(n_words, prefix, prefix_len, unk_id, max_runes, &rule)) != DTK_OK) return rc;
  // pieces beyond cap are counted and not stored; an unknown token's single piece replaces whatever was stored
  uint32_t n = dtk_wp_split(img.view, rule, DtkWpBytesKey{key, (uint32_t)key_len}, [&](uint32_t k, int32_t id, uint32_t end) {
    if (k < cap) { ids[k] = id; ends[k] = end; }
  });
  if (n == DTK_WP_BAD) {
    n = 1;
    if (cap) { ids[0] = unk_id; ends[0] = (uint32_t)key_len; }
  }
  *n_out = n;
  return n > cap ? DTK_E_CAPACITY : DTK_OK;
}

// K is valid UTF-8 (what the replacement leaves)
static bool valid_key(const uint8_t *key, uint32_t n) {
  for (uint32_t i = 0; i < n;) {
    const uint32_t c = key[i];
    if (c < 0x80u) { i++; continue; }
    if (c < 0xC0u) return false;
    const uint32_t cp = dtk_utf8_lead([&](uint32_t j) { return (uint32_t)key[j]; }, i, n, c);
    if (cp == 0xFFFDu && !(n - i >= 3u && c == 0xEFu && key[i + 1] == 0xBFu && key[i + 2] == 0xBDu)) return false;  // (U+FFFD itself is fine)
    i += cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u;
  }
  return true;
}

extern "C" int dtk_wordpiece_probe_fold_mem(const uint8_t *bytes, const uint64_t *off, uint32_t n_words, const uint8_t *prefix,
                                            uint32_t prefix_len, int32_t unk_id, uint32_t max_runes, const uint32_t *from,
                                            const uint32_t *to_off, const uint32_t *to, uint32_t n_fold, const uint8_t *key,
                                            size_t key_len, int32_t *ids, uint32_t *ends, uint32_t cap, uint32_t *n_out) {
  if (!n_out || (key_len && !key) || key_len >= (1ull << 32) || (cap && (!ids || !ends))) return DTK_E_ARG;
  VocabImage img;
  FoldImage fold;
  DtkWpRule rule;
  int rc = build_image(bytes, off, n_words, img);
  if (rc != DTK_OK || (rc = wordpiece_rule(n_words, prefix, prefix_len, unk_id, max_runes, &rule)) != DTK_OK ||
      (rc = fold_image(from, to_off, to, n_fold, fold)) != DTK_OK)
    return rc;
  if (!valid_key(key, (uint32_t)key_len)) return DTK_E_ARG;
  const DtkFoldDev F = fold.view(fold.words.data());
  const DtkFoldedKey<DtkWpBytesKey> folded{DtkWpBytesKey{key, (uint32_t)key_len}, F, F.entry};
  uint32_t n = dtk_wp_split(img.view, rule, folded, [&](uint32_t k, int32_t id, uint32_t end) {
    if (k < cap) { ids[k] = id; ends[k] = end; }
  });
  if (n == DTK_WP_BAD) {
    n = 1;
    if (cap) { ids[0] = unk_id; ends[0] = (uint32_t)key_len; }
  }
  *n_out = n;
  return n > cap ? DTK_E_CAPACITY : DTK_OK;
}

extern "C" int dtk_vocab_probe_mem(const uint8_t *bytes, const uint64_t *off, uint32_t n_words, const uint8_t *key,
                                   size_t key_len, int32_t *id) {
  if (!id || (key_len && !key)) return DTK_E_ARG;
  VocabImage img;
  const int rc = build_image(bytes, off, n_words, img);
  if (rc != DTK_OK) return rc;
  *id = find_key(img.view, key, key_len, nullptr);
  return DTK_OK;
}

extern "C" int dtk_vocab_create(const uint8_t *bytes, const uint64_t *off, uint32_t n_words, dtk_vocab **out) {
  if (!out) return DTK_E_ARG;
  *out = nullptr;
  VocabImage img;
  int rc = build_image(bytes, off, n_words, img);
  if (rc != DTK_OK) return rc;
  if (dtk_device_count() <= 0) return DTK_E_NO_DEVICE;
  std::unique_ptr<dtk_vocab> v(new dtk_vocab());
  HIP_TRY(hipGetDevice(&v->device));
  v->n_words = n_words;
  const uint64_t n_slots = img.slots.size(), n_bytes = off[n_words], byte_words = n_bytes / 4 + 1;
  if ((rc = v->d_slots.fit(n_slots, n_slots)) || (rc = v->d_off.fit((uint64_t)n_words + 1, (uint64_t)n_words + 1)) ||
      (rc = v->d_bytes.fit(byte_words, byte_words)))
    return rc;
  HIP_TRY(hipMemcpy(v->d_slots.p, img.slots.data(), n_slots * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(v->d_off.p, img.off.data(), ((size_t)n_words + 1) * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(v->d_bytes.p, 0, byte_words * 4));
  if (n_bytes) HIP_TRY(hipMemcpy(v->d_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice));
  v->dev = DtkVocabDev{v->d_slots.p, v->d_off.p, reinterpret_cast<const uint8_t *>(v->d_bytes.p), img.view.mask, n_words,
                       img.view.hash_bits, img.view.max_word};
  *out = v.release();
  return DTK_OK;
}

extern "C" void dtk_vocab_free(dtk_vocab *v) { delete v; }

extern "C" uint32_t dtk_vocab_size(const dtk_vocab *v) { return v ? v->n_words : 0u; }

extern "C" int dtk_tally_create(const dtk_vocab *v, dtk_tally **out) {
  if (!out) return DTK_E_ARG;
  *out = nullptr;
  if (!v) return DTK_E_ARG;
  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  if (device != v->device) return DTK_E_ARG;  // (the counters live beside their vocabulary)
  std::unique_ptr<dtk_tally> t(new dtk_tally());
  t->device = device;
  t->n_words = v->n_words;
  const uint64_t n = (uint64_t)v->n_words + 1;
  int rc = t->d_counts.fit(n, n);
  if (rc != DTK_OK) return rc;
  HIP_TRY(hipMemset(t->d_counts.p, 0, n * 8));
  *out = t.release();
  return DTK_OK;
}

// (Both wait for the device's earlier work on the null stream's terms only: the lookups whose batch has been waited
//  for are complete, and those are the ones the sum is defined over.)
extern "C" int dtk_tally_read(dtk_tally *t, uint64_t *counts) {
  if (!t || !counts) return DTK_E_ARG;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the kernel's counters are the header's");
  HIP_TRY(hipMemcpy(counts, t->d_counts.p, ((size_t)t->n_words + 1) * 8, hipMemcpyDeviceToHost));
  return DTK_OK;
}

extern "C" int dtk_tally_reset(dtk_tally *t) {
  if (!t) return DTK_E_ARG;
  HIP_TRY(hipMemset(t->d_counts.p, 0, ((size_t)t->n_words + 1) * 8));
  return DTK_OK;
}

extern "C" void dtk_tally_free(dtk_tally *t) { delete t; }
