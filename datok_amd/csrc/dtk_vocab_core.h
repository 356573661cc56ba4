// dtk_vocab_core.h -- the vocabulary table's one definition, for the host and for gfx950: the hash over a key's bytes,
// how a slot and a tag follow from it, the probe step, and the probe loop itself.  The builder and dtk_vocab_probe_mem
// (dtk_vocab.cpp) and the lookup kernel (dtk_tokenid.hip) all go through these functions, so they cannot drift apart.
//
// The table is open-addressed with linear probing.  A slot is 8 bytes: a non-zero 32-bit tag from the hash's high half
// in the low word, the word's index in the high word; 0 is an empty slot.  The slot count is a power of two and at
// least twice the word count (and at least 2), so a probe always meets an empty slot.  A tag match alone decides
// nothing: the caller's `eq` compares the bytes.  Of equal words only the lowest index is in the table.
#pragma once
#include <stdint.h>

#include "dtk_fold_core.h"  // (DTK_VH, and the fold of the lookup's arguments)

struct DtkVocabDev {
  const uint64_t *slots;  // mask + 1
  const uint32_t *off;    // n_words + 1: word w is bytes[off[w] .. off[w + 1])
  const uint8_t *bytes;   // (allocated in whole 32-bit words)
  uint32_t mask;          // slots - 1
  uint32_t n_words;
  int32_t hash_bits;      // test hook VOCAB_HASH_BITS as it stood when the table was built: >= 0 keeps the hash's low bits
  uint32_t max_word;      // the longest word's bytes: no longer key can match (the bound of dtk_wordpiece_core.h's candidates)
};

// The hash: two 32-bit lanes fed byte by byte (FNV-1a, and a Murmur3-style rotate-multiply), folded with the length
// through a 64-bit finaliser.  Byte-wise, because the kernel's replacement path produces its key a byte at a time.
struct DtkVocabHash { uint32_t a, b; };
DTK_VH DtkVocabHash dtk_vh_init() { return DtkVocabHash{0x811C9DC5u, 0x9E3779B9u}; }
DTK_VH void dtk_vh_byte(DtkVocabHash &h, uint32_t c) {
  h.a = (h.a ^ c) * 0x01000193u;
  const uint32_t x = h.b ^ (c * 0xCC9E2D51u);
  h.b = ((x << 13) | (x >> 19)) * 5u + 0xE6546B64u;
}
DTK_VH uint64_t dtk_vh_finish(const DtkVocabHash &h, uint64_t len, int32_t hash_bits) {
  uint64_t x = (((uint64_t)h.b << 32) | h.a) ^ (len * 0x9E3779B97F4A7C15ull);
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  if (hash_bits >= 0 && hash_bits < 64) x &= (1ull << hash_bits) - 1u;
  return x;
}
DTK_VH uint32_t dtk_vh_tag(uint64_t h) { const uint32_t t = (uint32_t)(h >> 32); return t ? t : 1u; }
DTK_VH uint32_t dtk_vh_slot(uint64_t h, uint32_t mask) { return (uint32_t)h & mask; }
DTK_VH uint32_t dtk_vh_next(uint32_t slot, uint32_t mask) { return (slot + 1u) & mask; }
DTK_VH uint64_t dtk_vh_entry(uint64_t h, uint32_t word) { return ((uint64_t)word << 32) | dtk_vh_tag(h); }

// The word equal to the key with hash h, or -1.  eq(w): the key's bytes are word w's.  *free_slot (may be null): the
// empty slot that ended an unsuccessful probe -- where the builder puts the key.
template <class Eq>
DTK_VH int32_t dtk_vocab_find(const DtkVocabDev &V, uint64_t h, Eq eq, uint32_t *free_slot) {
  const uint32_t tag = dtk_vh_tag(h);
  for (uint32_t s = dtk_vh_slot(h, V.mask);; s = dtk_vh_next(s, V.mask)) {
    const uint64_t e = V.slots[s];
    if (e == 0) {
      if (free_slot) *free_slot = s;
      return -1;
    }
    if ((uint32_t)e == tag && eq((uint32_t)(e >> 32))) return (int32_t)(e >> 32);
  }
}

// ---- the lookup kernel's arguments (dtk_tokenid.hip)
struct DtkTokenIdArgs {
  const uint8_t *text;           // the batch's input; nothing beyond the aligned word of its last byte is read
  uint64_t total;
  const uint64_t *doc_off;       // n_docs + 1
  uint32_t n_docs;
  const uint64_t *tok_off;       // n_docs + 1
  const uint32_t *tok_bstart, *tok_bend;
  uint64_t n_tok;
  const void *sym_base;          // the run's symbol stream (DtkSym), non-null only if the run saw invalid UTF-8
  const uint16_t *sym_lut;
  struct DtkVocabDev vocab;
  struct DtkFoldDev fold;        // entry == null: no fold
  int32_t *tok_id;               // n_tok
  unsigned long long *n_unknown; // device word, cleared in front of the launch
  unsigned long long *tally;     // n_words + 1 counters (the last: unknown), or null
};
extern "C" int dtk_launch_token_ids(const DtkTokenIdArgs *args, void *stream);
