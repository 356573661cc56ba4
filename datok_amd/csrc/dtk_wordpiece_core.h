// dtk_wordpiece_core.h -- the WordPiece rule's one definition (include/datok_gpu.h, dtk_batch_set_wordpiece), for the
// host and for gfx950: dtk_wordpiece_probe_mem (dtk_vocab.cpp) and the kernels of dtk_wordpiece.hip call dtk_wp_split,
// so they cannot drift apart.  It rests on the table, the hash and the probe loop of dtk_vocab_core.h.
//
// A key is read through its SOURCE bytes: key.size() of them, and key.at(i) is byte i or DTK_WP_REPLACED for a byte
// that does not decode and stands in the key as EF BF BD.  A replaced byte is a rune of its own, so every rune boundary
// of the key is a boundary between source bytes, and the rule runs in source offsets throughout: that is what
// piece_bend reports.  (The host probe's key is the key after replacement: source and key bytes are the same there.)
//
// Search order: the whole remainder first -- one forward pass over its bytes and one probe, which for a token that is a
// word is exactly the lookup of dtk_tokenid.hip -- and only when that misses a second forward pass that probes at every
// rune boundary and remembers the last hit.  The hash is byte-wise, so one pass yields the hash of every prefix of the
// remainder, and the state behind the continuation prefix is computed once, on the host (DtkWpRule::pre).  Candidates
// longer than the vocabulary's longest word are never hashed.
#pragma once
#include <stdint.h>

#include "dtk_fold_core.h"
#include "dtk_vocab_core.h"

#define DTK_WP_REPLACED 0x100u    // Key::at: the byte prints as EF BF BD
#define DTK_WP_BAD 0xFFFFFFFFu    // dtk_wp_split: the token is the single piece unk_id
#define DTK_WP_MAX_PREFIX 16u
#define DTK_WP_DEFAULT_RUNES 100u // BERT's max_input_chars_per_word

struct DtkWpRule {
  DtkVocabHash pre;                   // the hash's state behind the prefix
  uint8_t prefix[DTK_WP_MAX_PREFIX];  // what a continuation word begins with
  uint32_t prefix_len;
  int32_t unk_id;
  uint32_t max_runes;                 // (never 0 here: the default has been filled in)
};

DTK_VH DtkWpRule dtk_wp_rule(const uint8_t *prefix, uint32_t prefix_len, int32_t unk_id, uint32_t max_runes) {
  DtkWpRule r{};
  r.pre = dtk_vh_init();
  for (uint32_t k = 0; k < prefix_len && k < DTK_WP_MAX_PREFIX; k++) {
    r.prefix[k] = prefix[k];
    dtk_vh_byte(r.pre, prefix[k]);
  }
  r.prefix_len = prefix_len;
  r.unk_id = unk_id;
  r.max_runes = max_runes ? max_runes : DTK_WP_DEFAULT_RUNES;
  return r;
}

DTK_VH bool dtk_wp_rune_start(uint32_t c) { return c == DTK_WP_REPLACED || (c & 0xC0u) != 0x80u; }

// one source byte into the hash; len: the key bytes hashed so far
DTK_VH void dtk_wp_feed(DtkVocabHash &h, uint32_t c, uint32_t &len) {
  if (c == DTK_WP_REPLACED) {
    dtk_vh_byte(h, 0xEFu); dtk_vh_byte(h, 0xBFu); dtk_vh_byte(h, 0xBDu);
    len += 3u;
  } else {
    dtk_vh_byte(h, c);
    len++;
  }
}

// What the rule asks of a key, source position by source position: DtkWpOps<Key>.  In general a source RUNE gives 0 to
// DTK_FOLD_MAX_BYTES key bytes, all of them at the position of its first byte, and the positions of its other bytes
// give nothing.  This is the form for a key that is read byte by byte (size(), at(i)): a byte is itself, a replaced one
// is EF BF BD.  DtkFoldedKey below has the other form.
//   folds           some source runes may give no key byte, or several runes
//   start(key, i)   a source rune begins at position i
//   runes(key, i)   the key's runes that position i gives
//   feed(key, i, h, len)    position i's key bytes into the hash, and counted
//   same(key, i, p, k)      position i's key bytes are p[k ..); k moves behind them
template <class Key>
struct DtkWpOps {
  static constexpr bool folds = false;
  static DTK_VH bool start(const Key &key, uint32_t i) { return dtk_wp_rune_start(key.at(i)); }
  static DTK_VH uint32_t runes(const Key &key, uint32_t i) { return dtk_wp_rune_start(key.at(i)) ? 1u : 0u; }
  static DTK_VH void feed(const Key &key, uint32_t i, DtkVocabHash &h, uint32_t &len) { dtk_wp_feed(h, key.at(i), len); }
  static DTK_VH bool same(const Key &key, uint32_t i, const uint8_t *p, uint32_t &k) {
    const uint32_t c = key.at(i);
    if (c == DTK_WP_REPLACED) {
      if (p[k] != 0xEFu || p[k + 1u] != 0xBFu || p[k + 2u] != 0xBDu) return false;
      k += 3u;
    } else {
      if (p[k] != c) return false;
      k++;
    }
    return true;
  }
};

// Word w is the candidate: the prefix (start != 0) and the key of source positions [start, end), len bytes in all.
template <class Key>
DTK_VH bool dtk_wp_equal(const DtkVocabDev &V, const DtkWpRule &R, uint32_t w, const Key &key, uint32_t start, uint32_t end,
                         uint32_t len) {
  const uint32_t o = V.off[w];
  if (V.off[w + 1u] - o != len) return false;
  const uint8_t *p = V.bytes + o;  // (every index below is < len: len was counted over the same bytes)
  uint32_t k = 0;
  if (start)
    for (; k < R.prefix_len; k++)
      if (p[k] != R.prefix[k]) return false;
  for (uint32_t i = start; i < end; i++)
    if (!DtkWpOps<Key>::same(key, i, p, k)) return false;
  return true;
}

template <class Key>
DTK_VH int32_t dtk_wp_find(const DtkVocabDev &V, const DtkWpRule &R, const DtkVocabHash &h, const Key &key, uint32_t start,
                           uint32_t end, uint32_t len) {
  return dtk_vocab_find(
      V, dtk_vh_finish(h, len, V.hash_bits), [&](uint32_t w) { return dtk_wp_equal(V, R, w, key, start, end, len); }, nullptr);
}

// The pieces of one key, in order: emit(k, id, end) with end the piece's end in source bytes.  Returns their number, or
// DTK_WP_BAD: too many runes or a remainder no word begins -- whatever was emitted before does not count then.
// len counts KEY bytes: under a fold it is the folded candidate's length that V.max_word bounds, and a candidate that
// has no key byte behind the prefix is never probed.
template <class Key, class Emit>
DTK_VH uint32_t dtk_wp_split(const DtkVocabDev &V, const DtkWpRule &R, const Key &key, Emit emit) {
  using Ops = DtkWpOps<Key>;
  const uint32_t n = key.size();
  // (a rune has at least one source byte, and a source rune gives at most DTK_FOLD_MAX of the key's)
  if ((uint64_t)n * (Ops::folds ? DTK_FOLD_MAX : 1u) > R.max_runes) {
    uint32_t runes = 0;
    for (uint32_t i = 0; i < n; i++) runes += Ops::runes(key, i);
    if (runes > R.max_runes) return DTK_WP_BAD;
  }
  uint32_t start = 0, k = 0;
  while (start < n) {
    const DtkVocabHash h0 = start ? R.pre : dtk_vh_init();
    const uint32_t len0 = start ? R.prefix_len : 0u;
    int32_t hit = -1;
    uint32_t hit_end = n;
    {  // the whole remainder
      DtkVocabHash h = h0;
      uint32_t len = len0;
      for (uint32_t i = start; i < n && len <= V.max_word; i++) Ops::feed(key, i, h, len);
      if (len <= V.max_word && !(Ops::folds && len == len0)) hit = dtk_wp_find(V, R, h, key, start, n, len);
    }
    if (hit < 0) {  // every shorter candidate, forward: the last hit is the longest
      DtkVocabHash h = h0;
      uint32_t len = len0, probed = len0;  // probed: the length of the candidate probed last (folds only)
      int32_t last = -1;                   // ... and what the probe gave
      for (uint32_t i = start; i + 1u < n;) {
        Ops::feed(key, i, h, len);
        i++;
        if (len > V.max_word) break;
        if (!Ops::start(key, i)) continue;
        int32_t id;
        if (Ops::folds && len == probed) {
          id = last;  // (the runes since then folded to nothing: the same candidate, a later end)
        } else {
          id = dtk_wp_find(V, R, h, key, start, i, len);
          if (Ops::folds) { probed = len; last = id; }
        }
        if (id >= 0) { hit = id; hit_end = i; }
      }
      if (hit < 0) return DTK_WP_BAD;
    }
    emit(k++, hit, hit_end);
    start = hit_end;
  }
  return k;
}

// The host probe's key, and any key held as its bytes after replacement.
struct DtkWpBytesKey {
  const uint8_t *p;
  uint32_t n;
  DTK_VH uint32_t size() const { return n; }
  DTK_VH uint32_t at(uint32_t i) const { return p[i]; }
};

// A key under a fold (dtk_fold_core.h): F applied to the runes of Inner's key -- a key read byte by byte, whose
// replaced bytes are U+FFFD -- where they are read.  Positions are Inner's source bytes, so cuts and piece ends stay in
// source bytes.  A rune is decoded once, at its first byte; an ASCII byte takes its entry from `ascii`, the caller's
// copy of the table's block 0 (the kernels': in LDS), and one that folds to itself or to another ASCII byte touches
// nothing else.
template <class Inner>
struct DtkFoldedKey {
  Inner in;
  DtkFoldDev F;
  const uint32_t *ascii;
  DTK_VH uint32_t size() const { return in.size(); }
  // position i's key bytes, each into put(byte); returns the runes they are
  template <class Put>
  DTK_VH uint32_t each(uint32_t i, Put put) const {
    const uint32_t c = in.at(i);
    uint32_t cp = c, e;
    if (c < 0x80u) {
      e = ascii[c];
      if (e <= 0x80u) { put(e ? e - 1u : c); return 1u; }
    } else {
      if (c == DTK_WP_REPLACED) cp = 0xFFFDu;
      else if (c < 0xC0u) return 0u;  // a continuation byte: its rune was read at its first byte
      else cp = dtk_utf8_lead([&](uint32_t j) { return in.at(j); }, i, in.size(), c);
      e = dtk_fold_entry(F, ascii, cp);
      if (e == 0u) {  // itself: the source bytes again (U+FFFD for a replaced byte)
        dtk_utf8_put(cp, put);
        return 1u;
      }
    }
    uint32_t to[DTK_FOLD_MAX];
    const uint32_t n = dtk_fold_expand(F, e, cp, to);
    for (uint32_t k = 0; k < n; k++) dtk_utf8_put(to[k], put);
    return n;
  }
  // the whole key's hash and length, and its comparison with a word of that length (dtk_tokenid.hip's lookup)
  DTK_VH uint64_t hash(int32_t hash_bits, uint32_t *len) const {
    DtkVocabHash h = dtk_vh_init();
    uint32_t k = 0;
    const uint32_t n = in.size();
    for (uint32_t i = 0; i < n; i++) each(i, [&](uint32_t b) { dtk_vh_byte(h, b); k++; });
    *len = k;
    return dtk_vh_finish(h, k, hash_bits);
  }
  DTK_VH bool equals(const uint8_t *word, uint32_t len) const {
    uint32_t k = 0;
    bool ok = true;
    const uint32_t n = in.size();
    for (uint32_t i = 0; i < n && ok; i++) each(i, [&](uint32_t b) { ok = ok && k < len && word[k] == b; k++; });
    return ok && k == len;
  }
};

template <class Inner>
struct DtkWpOps<DtkFoldedKey<Inner>> {
  using Key = DtkFoldedKey<Inner>;
  static constexpr bool folds = true;
  static DTK_VH bool start(const Key &key, uint32_t i) { return dtk_wp_rune_start(key.in.at(i)); }
  static DTK_VH uint32_t runes(const Key &key, uint32_t i) { return key.each(i, [](uint32_t) {}); }
  static DTK_VH void feed(const Key &key, uint32_t i, DtkVocabHash &h, uint32_t &len) {
    key.each(i, [&](uint32_t b) { dtk_vh_byte(h, b); len++; });
  }
  static DTK_VH bool same(const Key &key, uint32_t i, const uint8_t *p, uint32_t &k) {
    bool ok = true;  // (k stays below the candidate's length, which was counted over these bytes)
    key.each(i, [&](uint32_t b) { ok = ok && p[k] == b; k++; });
    return ok;
  }
};

// ---- the kernels' arguments (dtk_wordpiece.hip)
#define DTK_WP_TILE 256u  // tokens of one block round: a scan tile
struct DtkWpFirst { int32_t id; uint32_t bend; };  // a token's first piece, as piece_id / piece_bend take it
struct DtkWordPieceArgs {
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
  struct DtkWpRule rule;
  struct DtkFoldDev fold;        // entry == null: no fold
  uint64_t *tile_base;           // workspace, tiles + 1: a tile's pieces, then their exclusive scan and the total
  struct DtkWpFirst *first;      // workspace, n_tok: the first pass's note for the second
  unsigned long long *cnt;       // device words [n_pieces, n_unknown], cleared in front of the launch
  uint64_t *piece_off;           // n_tok + 1
  int32_t *piece_id;             // cap
  uint32_t *piece_bend;          // cap
  uint64_t cap;                  // with more pieces than this none is written (the counters and piece_off are)
};
DTK_VH uint64_t dtk_wp_tiles(uint64_t n_tok) { return (n_tok + DTK_WP_TILE - 1u) / DTK_WP_TILE; }
extern "C" int dtk_launch_wordpiece(const DtkWordPieceArgs *args, void *stream);
