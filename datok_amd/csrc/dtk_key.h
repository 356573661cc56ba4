// dtk_key.h -- a token's key on the device, for the kernels that look tokens up in a vocabulary (dtk_tokenid.hip,
// dtk_wordpiece.hip): the surface as the reference's writer prints it, the document's bytes [tok_bstart, tok_bend) with
// every byte that does not decode replaced by EF BF BD.  A run without invalid UTF-8 never touches the symbol stream:
// its keys are the text's bytes, read as aligned 32-bit words (the last word read is the one that holds the key's last
// byte).  With invalid bytes in the run the key is produced a byte at a time under the renderers' rule
// (sym_invalid_byte).
#pragma once
#include <hip/hip_runtime.h>

#include "dtk_device.h"
#include "dtk_vocab_core.h"
#include "dtk_wordpiece_core.h"

namespace {
// Bytes [at, at + n) of a buffer, read as the aligned 32-bit words that hold them: nothing in front of the word of the
// first byte and nothing behind the word of the last one is touched.
struct WordReader {
  const uint32_t *w;
  uint32_t cur, sh;
  __device__ __forceinline__ WordReader(const uint8_t *p, uint32_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3u);
    sh = (uint32_t)(a & 3u) * 8u;
    cur = n ? *w : 0u;
  }
  // the next byte; more: another byte follows it
  __device__ __forceinline__ uint32_t next(bool more) {
    const uint32_t c = (cur >> sh) & 0xFFu;
    sh += 8u;
    if (sh == 32u && more) { cur = *++w; sh = 0u; }
    return c;
  }
};

// The key of a run without invalid bytes: the text's bytes themselves.
struct RawKey {
  const uint8_t *p;
  uint32_t n;
  // The source-byte view of dtk_wordpiece_core.h: byte i through the aligned word that holds it.  The rule reads a
  // key's bytes in ascending runs, so the last word stays in a register: one load per four bytes, not one per byte.
  mutable uintptr_t held_at = 0;
  mutable uint32_t held = 0;
  __device__ __forceinline__ uint32_t size() const { return n; }
  __device__ __forceinline__ uint32_t at(uint32_t i) const {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p) + i, w = a & ~(uintptr_t)3u;
    if (w != held_at) { held = *reinterpret_cast<const uint32_t *>(w); held_at = w; }
    return (held >> ((uint32_t)(a & 3u) * 8u)) & 0xFFu;
  }
  __device__ __forceinline__ uint64_t hash(int32_t hash_bits, uint32_t *len) const {
    DtkVocabHash h = dtk_vh_init();
    WordReader r(p, n);
    for (uint32_t i = 0; i < n; i++) dtk_vh_byte(h, r.next(i + 1u < n));
    *len = n;
    return dtk_vh_finish(h, n, hash_bits);
  }
  __device__ __forceinline__ bool equals(const uint8_t *word, uint32_t len) const {  // (len == the key's length)
    WordReader a(p, len), b(word, len);
    for (uint32_t i = 0; i < len; i++)
      if (a.next(i + 1u < len) != b.next(i + 1u < len)) return false;
    return true;
  }
};

// The key of a run with invalid bytes: each of them leaves as EF BF BD (the rule of dtk_render.hip).
struct ReplacedKey {
  const uint8_t *p;
  uint32_t n;
  DtkSym S;
  uint64_t sy;  // the stream entry of p[0]
  __device__ __forceinline__ uint32_t size() const { return n; }
  __device__ __forceinline__ uint32_t at(uint32_t i) const { return sym_invalid_byte(S, sy + i) ? DTK_WP_REPLACED : p[i]; }
  __device__ __forceinline__ uint64_t hash(int32_t hash_bits, uint32_t *len) const {
    DtkVocabHash h = dtk_vh_init();
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (sym_invalid_byte(S, sy + i)) {
        dtk_vh_byte(h, 0xEFu); dtk_vh_byte(h, 0xBFu); dtk_vh_byte(h, 0xBDu);
        k += 3u;
      } else {
        dtk_vh_byte(h, p[i]);
        k++;
      }
    }
    *len = k;
    return dtk_vh_finish(h, k, hash_bits);
  }
  __device__ __forceinline__ bool equals(const uint8_t *word, uint32_t len) const {
    uint32_t k = 0;
    for (uint32_t i = 0; i < n; i++) {
      if (sym_invalid_byte(S, sy + i)) {
        if (word[k] != 0xEFu || word[k + 1u] != 0xBFu || word[k + 2u] != 0xBDu) return false;
        k += 3u;
      } else {
        if (word[k] != p[i]) return false;
        k++;
      }
    }
    return k == len;
  }
};

// Either of them under a fold (dtk_batch_set_fold): the rule's own DtkFoldedKey, read through Inner::at -- for RawKey
// the aligned words, so nothing behind the word of the key's last byte is read whatever that byte folds to.  `ascii` is
// the block's LDS copy of the fold's ASCII page (stage_fold_ascii).
template <class Inner>
using FoldedKey = DtkFoldedKey<Inner>;

// The fold's ASCII page into the block's LDS, once per block: the entry of an ASCII byte -- nearly every byte of running
// text -- then costs an LDS read and no dependent global load.  Every thread of the block calls it.
__device__ __forceinline__ void stage_fold_ascii(const DtkFoldDev &F, uint32_t *ascii) {
  for (uint32_t j = threadIdx.x; j < DTK_FOLD_PAGE; j += blockDim.x) ascii[j] = F.entry[j];
  __syncthreads();
}

}  // namespace
