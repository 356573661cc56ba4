// dtk_wordpiece.hip -- every token of a finished run split into WordPiece ids (dtk_batch_set_wordpiece, include/datok_gpu.h):
// greedy longest-match-first over the token's key, continuation pieces looked up behind the prefix.  The rule itself is
// dtk_wp_split of dtk_wordpiece_core.h, the code the host probe runs; the keys are those of dtk_tokenid.hip (dtk_key.h).
// With a fold attached (dtk_batch_set_fold) the keys are read through FoldedKey; piece ends stay in source bytes.
// Runs on the download stream behind finish(), so the token count is final and repairs and the exact pass are done.
//
// Three launches, blocks of 256 threads over tiles of 256 tokens, one lane per token:
//   k_wp_count   the lane finds its document, runs the rule and keeps only the piece count; the block scans its tile
//                (block_excl_scan64): piece_off[i] becomes the pieces in front of token i inside its tile, tile_base[t]
//                the tile's pieces.  The unknown tokens of a wave go to the counter with one atomic per wave.
//   k_wp_scan    one block: tile_base becomes its exclusive scan (scan_row64), the total goes behind it, into the
//                counter block and into piece_off[n_tok].
//   k_wp_write   piece_off[i] gets its tile's base added.  A token of one piece -- most tokens of running text -- takes it
//                from the 8 bytes the first pass left per token (first[i]: the first piece's id and end); a lane with
//                more runs the rule again and writes them at its offset.  Nothing per text byte is kept between the
//                passes.  With more pieces than the output block holds (args.cap) no piece is written; the host sees
//                the total, grows the block and runs the three again.
#include <hip/hip_runtime.h>

#include "dtk_internal.h"
#include "dtk_device.h"
#include "dtk_key.h"
#include "dtk_wordpiece_core.h"

#define DTK_WP_MAX_BLOCKS 2048u
static_assert(DTK_WP_TILE == 256u, "a tile is a block's threads: the block scans of dtk_device.h");

namespace {
// Token i's row: where its key lies, clamped to its document.
struct WpRow {
  uint64_t d0;       // the document's first byte in the text
  uint32_t bs, be;   // the key's source bytes in the document (clamped); be: where an unknown piece ends
  bool key;          // false: tok_bstart > tok_bend, a row the reference cannot print
};

__device__ __forceinline__ WpRow wp_row(const DtkWordPieceArgs &a, uint64_t i) {
  // the token's document: the last d with tok_off[d] <= i (documents without a token have equal neighbours)
  uint32_t lo = 0, hi = a.n_docs;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.tok_off[mid] <= i) lo = mid; else hi = mid;
  }
  const uint64_t d0 = a.doc_off[lo], d1 = a.doc_off[lo + 1u];
  const uint64_t len = d1 > d0 && d1 <= a.total ? d1 - d0 : 0u;
  uint64_t bs = a.tok_bstart[i], be = a.tok_bend[i];
  const bool key = bs <= be;
  // rows of flagged documents are clamped to the document: nothing outside its bytes is read
  if (be > len) be = len;
  if (bs > be) bs = be;
  return WpRow{d0, (uint32_t)bs, (uint32_t)be, key};
}

// FOLD: the launch has a fold attached (dtk_batch_set_fold) and every key is read through it, with the fold's ASCII
// page in the block's LDS (ascii); chosen per launch, so the kernels of a run without a fold are the ones they were.
template <bool FOLD, class Emit>
__device__ __forceinline__ uint32_t wp_split(const DtkWordPieceArgs &a, const WpRow &r, const uint32_t *ascii, Emit emit) {
  const uint8_t *p = a.text + r.d0 + r.bs;
  const uint32_t n = r.be - r.bs;
  if constexpr (FOLD) {
    if (a.sym_base)
      return dtk_wp_split(a.vocab, a.rule,
                          FoldedKey<ReplacedKey>{ReplacedKey{p, n, DtkSym{a.sym_base, a.sym_lut}, r.d0 + r.bs}, a.fold, ascii}, emit);
    return dtk_wp_split(a.vocab, a.rule, FoldedKey<RawKey>{RawKey{p, n}, a.fold, ascii}, emit);
  }
  if (a.sym_base) return dtk_wp_split(a.vocab, a.rule, ReplacedKey{p, n, DtkSym{a.sym_base, a.sym_lut}, r.d0 + r.bs}, emit);
  return dtk_wp_split(a.vocab, a.rule, RawKey{p, n}, emit);
}

template <bool FOLD>
__global__ __launch_bounds__(DTK_WP_TILE) void k_wp_count(const DtkWordPieceArgs a) {
  __shared__ uint64_t wave_tot[DTK_WP_TILE / WAVE];
  __shared__ uint32_t fold_ascii[FOLD ? DTK_FOLD_PAGE : 1u];
  if constexpr (FOLD) stage_fold_ascii(a.fold, fold_ascii);
  const uint64_t tiles = dtk_wp_tiles(a.n_tok);
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // (block-uniform: the scan and the ballot take every lane)
    const uint64_t i = t * DTK_WP_TILE + threadIdx.x;
    const bool live = i < a.n_tok;
    uint32_t c = 0;
    bool unknown = false;
    if (live) {
      const WpRow r = wp_row(a, i);
      int32_t id0 = 0;
      uint32_t end0 = 0;
      c = DTK_WP_BAD;
      if (r.key) c = wp_split<FOLD>(a, r, fold_ascii, [&](uint32_t k, int32_t id, uint32_t end) { if (k == 0u) { id0 = id; end0 = end; } });
      unknown = c == DTK_WP_BAD;
      if (unknown) c = 1u;
      // (what a token of one piece delivers: the word and where it ends, or unk_id and the clamped tok_bend)
      a.first[i] = DtkWpFirst{unknown ? a.rule.unk_id : id0, unknown ? r.be : r.bs + end0};
    }
    uint64_t sum;
    const uint64_t x = block_excl_scan64(c, wave_tot, sum);
    if (live) a.piece_off[i] = x;
    if (threadIdx.x == 0u) a.tile_base[t] = sum;
    const uint32_t n_unknown = popc(__ballot(unknown));
    if (lane_id() == 0u && n_unknown) atomicAdd(a.cnt + 1, (unsigned long long)n_unknown);
  }
}

__global__ __launch_bounds__(256) void k_wp_scan(const DtkWordPieceArgs a) {
  __shared__ uint64_t wave_tot[256 / WAVE];
  const uint32_t tiles = (uint32_t)dtk_wp_tiles(a.n_tok);
  const uint64_t sum = scan_row64(a.tile_base, tiles, wave_tot);
  if (threadIdx.x == 0u) {
    a.tile_base[tiles] = sum;
    a.piece_off[a.n_tok] = sum;
    a.cnt[0] = sum;
  }
}

template <bool FOLD>
__global__ __launch_bounds__(DTK_WP_TILE) void k_wp_write(const DtkWordPieceArgs a) {
  __shared__ uint32_t fold_ascii[FOLD ? DTK_FOLD_PAGE : 1u];
  if constexpr (FOLD) stage_fold_ascii(a.fold, fold_ascii);
  const uint64_t tiles = dtk_wp_tiles(a.n_tok);
  const bool fits = a.tile_base[tiles] <= a.cap;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t i = t * DTK_WP_TILE + threadIdx.x;
    const bool live = i < a.n_tok;
    const uint64_t base = a.tile_base[t];
    uint64_t x = 0, x1 = 0;
    if (live) {
      x = a.piece_off[i];
      // (the next token's, or the tile's pieces: tile_base[t + 1] - base)
      x1 = threadIdx.x + 1u < DTK_WP_TILE && i + 1u < a.n_tok ? a.piece_off[i + 1u] : a.tile_base[t + 1u] - base;
    }
    __syncthreads();  // every lane of the tile has read its neighbour's word
    if (!live) continue;
    const uint64_t o = base + x;
    a.piece_off[i] = o;
    const uint32_t c = (uint32_t)(x1 - x);
    if (!fits || c == 0u) continue;
    if (c == 1u) {
      const DtkWpFirst f = a.first[i];
      a.piece_id[o] = f.id;
      a.piece_bend[o] = f.bend;
      continue;
    }
    // (two pieces and more: the split is good and has a key)
    const WpRow r = wp_row(a, i);
    wp_split<FOLD>(a, r, fold_ascii, [&](uint32_t k, int32_t id, uint32_t end) {
      if (k < c) {  // (always: the first pass counted the same rule on the same bytes)
        a.piece_id[o + k] = id;
        a.piece_bend[o + k] = r.bs + end;
      }
    });
  }
}
}  // namespace

extern "C" int dtk_launch_wordpiece(const DtkWordPieceArgs *a, void *stream) {
  const uint64_t tiles = dtk_wp_tiles(a->n_tok);
  const uint32_t blocks = (uint32_t)(tiles < DTK_WP_MAX_BLOCKS ? tiles : DTK_WP_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  const bool fold = a->fold.entry != nullptr;
  if (blocks && fold) hipLaunchKernelGGL(k_wp_count<true>, dim3(blocks), dim3(DTK_WP_TILE), 0, s, *a);
  else if (blocks) hipLaunchKernelGGL(k_wp_count<false>, dim3(blocks), dim3(DTK_WP_TILE), 0, s, *a);
  hipLaunchKernelGGL(k_wp_scan, dim3(1), dim3(256), 0, s, *a);
  if (blocks && fold) hipLaunchKernelGGL(k_wp_write<true>, dim3(blocks), dim3(DTK_WP_TILE), 0, s, *a);
  else if (blocks) hipLaunchKernelGGL(k_wp_write<false>, dim3(blocks), dim3(DTK_WP_TILE), 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
