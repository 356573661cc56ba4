// dtk_encode.hip -- a finished run's sentences or documents as fixed-length model input rows (dtk_batch_set_encode,
// include/datok_gpu.h).  The rule is dtk_encode_core.h, the code dtk_encode_rows_mem runs on the host.  Runs on the
// download stream behind the WordPiece split and, for the sentence unit, behind the sentence table's launches.
//
// Three launches:
//   k_enc_count   blocks of 256 threads over tiles of 256 units, one lane per unit: the lane reads its token range
//                 (tok_off alone, or sen_off / sen_tok_end / tok_off), takes its pieces from piece_off, computes its
//                 windows and leaves the unit's numbers for the write (DtkEncUnit); the block scans its tile
//                 (block_excl_scan64).  The cut units of a wave go to the counter with one atomic per wave.
//   k_enc_scan    one block: tile_base becomes its exclusive scan (scan_row64); n_rows, n_units and the verdict `ok` go
//                 into the counter block.  ok is false when the split wrote no piece (it outgrew its block), when the
//                 sentence table was not written (it outgrew its bound), or with more rows than the output block holds:
//                 the write then stores nothing and the host encodes again.
//   k_enc_write   the hot path.  A group of G lanes (a power of two, 2..64, about max_len / 4) handles a run of up to
//                 eight consecutive rows (one, while longer runs would leave fewer than 8192 waves with work).  It
//                 finds the first row's unit by binary search -- the tile in tile_base, the unit among the tile's 256
//                 local offsets -- and steps from row to row without one (the unit's next window, or the next unit's
//                 first: every unit has a row).  So the work is dealt out by rows whatever the units' sizes, and a
//                 search's chain of dependent loads is paid once per run.  Everything about a row is uniform in the
//                 group.  A row is written in chunks of four positions that are 16-byte aligned in the table, one
//                 128-bit store per lane and chunk; a chunk that straddles a row's edge is stored position by
//                 position.  Narrow rows share a wave: with max_len = 5 a wave holds 32 rows.  word_id is one search
//                 in piece_off over the unit's tokens per body position.  The kernel's first grid-stride loop delivers
//                 unit_row_off from the two scan levels.
#include <hip/hip_runtime.h>

#include "dtk_internal.h"
#include "dtk_device.h"
#include "dtk_encode_core.h"

#define DTK_ENC_MAX_BLOCKS 4096u
#define DTK_ENC_RUN 8u        // consecutive rows of one group, at the most: one search for the first of them
#define DTK_ENC_WAVES 8192u   // ... and as few as it takes to have this many waves at work
static_assert(DTK_ENC_TILE == 256u, "a tile is a block's threads: the block scans of dtk_device.h");

namespace {
// units of the run, or 0 where the sentence table was not written
__device__ __forceinline__ uint64_t enc_units(const DtkEncodeArgs &a, bool &fits) {
  fits = true;
  if (a.rule.unit == DTK_ENCK_DOCUMENT) return a.n_docs;
  const uint64_t n = *a.sen_count;
  fits = n <= a.sen_cap && n <= a.units_cap;
  return fits ? n : 0u;
}

// Unit u's tokens, clamped to the run's token rows, and its document's first token.
__device__ __forceinline__ void enc_unit_tokens(const DtkEncodeArgs &a, uint64_t u, uint64_t &t0, uint64_t &t1, uint64_t &tok0) {
  if (a.rule.unit == DTK_ENCK_DOCUMENT) {
    t0 = tok0 = a.tok_off[u];
    t1 = a.tok_off[u + 1u];
  } else {
    // the row's document: the last d with sen_off[d] <= u (documents without a row have equal neighbours)
    uint32_t lo = 0, hi = a.n_docs;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (a.sen_off[mid] <= u) lo = mid; else hi = mid;
    }
    tok0 = a.tok_off[lo];
    t0 = tok0 + (u > a.sen_off[lo] ? a.sen_tok_end[u - 1u] : 0u);
    t1 = tok0 + a.sen_tok_end[u];
  }
  // (rows of flagged documents: nothing outside piece_off is read)
  if (t1 > a.n_tok) t1 = a.n_tok;
  if (t0 > t1) t0 = t1;
  if (tok0 > t0) tok0 = t0;
}

__global__ __launch_bounds__(DTK_ENC_TILE) void k_enc_count(const DtkEncodeArgs a) {
  __shared__ uint64_t wave_tot[DTK_ENC_TILE / WAVE];
  bool fits;
  const uint64_t n_units = enc_units(a, fits);
  const uint64_t tiles = dtk_enc_tiles(a.units_cap);
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // (block-uniform: the scan and the ballot take every lane)
    const uint64_t u = t * DTK_ENC_TILE + threadIdx.x;
    const bool live = u < n_units;
    uint64_t w = 0;
    bool cut = false;
    DtkEncUnit U{};
    if (live) {
      enc_unit_tokens(a, u, U.t0, U.t1, U.tok0);
      U.p0 = a.piece_off[U.t0];
      U.n = a.piece_off[U.t1] - U.p0;
      w = dtk_enc_windows(a.rule, U.n);
      cut = U.n > a.rule.body;
    }
    uint64_t sum;
    U.row_loc = block_excl_scan64(w, wave_tot, sum);
    if (live) a.unit[u] = U;
    if (threadIdx.x == 0u) a.tile_base[t] = sum;
    const uint32_t n_cut = popc(__ballot(cut));
    if (lane_id() == 0u && n_cut) atomicAdd(a.cnt + 1, (unsigned long long)n_cut);
  }
}

__global__ __launch_bounds__(256) void k_enc_scan(const DtkEncodeArgs a) {
  __shared__ uint64_t wave_tot[256 / WAVE];
  const uint32_t tiles = (uint32_t)dtk_enc_tiles(a.units_cap);
  const uint64_t sum = scan_row64(a.tile_base, tiles, wave_tot);
  if (threadIdx.x == 0u) {
    bool fits;
    const uint64_t n_units = enc_units(a, fits);
    a.tile_base[tiles] = sum;
    a.cnt[0] = sum;
    a.cnt[2] = n_units;
    a.cnt[3] = fits && a.piece_off[a.n_tok] <= a.piece_cap && sum <= a.rows_cap ? 1u : 0u;
  }
}

// Row r, window k of unit U, by lane j of the row's G lanes.
template <bool WORDS>
__device__ __forceinline__ void enc_write_row(const DtkEncodeArgs &a, const DtkEncRule &R, const DtkEncUnit &U, uint64_t k,
                                              uint64_t r, uint32_t j, uint32_t G) {
  uint64_t first;
  uint32_t len;
  dtk_enc_window(R, U.n, k, first, len);
  const uint64_t q0 = U.p0 + first;
  if (j == 0u) {
    a.row_len[r] = dtk_enc_row_len(R, len);
    a.row_piece0[r] = q0;
  }
  const int32_t *win = a.piece_id + q0;
  const uint64_t e0 = r * R.max_len, e1 = e0 + R.max_len;
  for (uint64_t ch = (e0 >> 2) + j; (ch << 2) < e1; ch += G) {
    const uint64_t e = ch << 2;
    int32_t v[4], x[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
      v[i] = 0; x[i] = -1;
      if (e + i < e0 || e + i >= e1) continue;
      const uint32_t p = (uint32_t)(e + i - e0);
      v[i] = dtk_enc_value(R, len, p, win);
      if (WORDS && dtk_enc_in_body(R, len, p)) x[i] = (int32_t)(dtk_enc_token(a.piece_off, U.t0, U.t1, q0 + (p - R.has_cls)) - U.tok0);
    }
    if (e >= e0 && e + 4u <= e1) {
      *reinterpret_cast<int4 *>(a.input_ids + e) = make_int4(v[0], v[1], v[2], v[3]);
      if (WORDS) *reinterpret_cast<int4 *>(a.word_id + e) = make_int4(x[0], x[1], x[2], x[3]);
    } else {  // (the chunk straddles the row's edge: its other positions are the neighbouring row's)
#pragma unroll
      for (uint32_t i = 0; i < 4u; i++) {
        if (e + i < e0 || e + i >= e1) continue;
        a.input_ids[e + i] = v[i];
        if (WORDS) a.word_id[e + i] = x[i];
      }
    }
  }
}

template <bool WORDS>
__global__ __launch_bounds__(256) void k_enc_write(const DtkEncodeArgs a, const uint32_t g_shift) {
  if (!a.cnt[3]) return;
  const uint64_t n_rows = a.cnt[0], n_units = a.cnt[2];
  for (uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x; u <= n_units; u += (uint64_t)gridDim.x * 256u)
    a.unit_row_off[u] = u < n_units ? a.tile_base[u / DTK_ENC_TILE] + a.unit[u].row_loc : n_rows;
  const DtkEncRule R = a.rule;
  const uint32_t G = 1u << g_shift, per_block = 256u >> g_shift;
  const uint32_t j = threadIdx.x & (G - 1u);
  const uint32_t tiles = (uint32_t)dtk_enc_tiles(n_units);
  // (few rows: a run of one each, so that the whole device writes; many: the search is paid once per eight)
  const uint64_t fill = n_rows / ((uint64_t)DTK_ENC_WAVES * (WAVE >> g_shift));
  const uint64_t run = fill < 1u ? 1u : fill > DTK_ENC_RUN ? DTK_ENC_RUN : fill;
  const uint64_t n_runs = (n_rows + run - 1u) / run;
  for (uint64_t c = (uint64_t)blockIdx.x * per_block + (threadIdx.x >> g_shift); c < n_runs; c += (uint64_t)gridDim.x * per_block) {
    uint64_t r = c * run;
    const uint64_t r_end = r + run < n_rows ? r + run : n_rows;
    // the first row's tile: the last t with tile_base[t] <= r (a tile without a row shares its base with its successor)
    uint32_t lo = 0, hi = tiles;
    while (hi - lo > 1u) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (a.tile_base[mid] <= r) lo = mid; else hi = mid;
    }
    const uint64_t in_tile = r - a.tile_base[lo];
    // ... and its unit: every unit has a row, so the local offsets ascend strictly
    uint64_t ulo = (uint64_t)lo * DTK_ENC_TILE, uhi = ulo + DTK_ENC_TILE < n_units ? ulo + DTK_ENC_TILE : n_units;
    while (uhi - ulo > 1u) {
      const uint64_t mid = ulo + ((uhi - ulo) >> 1);
      if (a.unit[mid].row_loc <= in_tile) ulo = mid; else uhi = mid;
    }
    // the run's further rows follow without a search: the unit's next window, or the next unit's first
    DtkEncUnit U = a.unit[ulo];
    uint64_t k = in_tile - U.row_loc, w = dtk_enc_windows(R, U.n);
    for (; r < r_end; r++) {
      enc_write_row<WORDS>(a, R, U, k, r, j, G);
      if (++k == w && r + 1u < r_end) {  // (a row behind this one exists, so a unit behind this one does)
        U = a.unit[++ulo];
        k = 0;
        w = dtk_enc_windows(R, U.n);
      }
    }
  }
}
}  // namespace

extern "C" int dtk_launch_encode(const DtkEncodeArgs *a, void *stream) {
  if (((uintptr_t)a->input_ids | (uintptr_t)a->word_id) & 15u) return -1;  // (the 128-bit stores)
  const uint64_t tiles = dtk_enc_tiles(a->units_cap);
  const uint32_t blocks = (uint32_t)(tiles < DTK_ENC_MAX_BLOCKS ? tiles : DTK_ENC_MAX_BLOCKS);
  // lanes per row: the row's chunks of four positions, as a power of two
  uint32_t g_shift = 1;
  while (g_shift < 6u && (4u << g_shift) < a->rule.max_len) g_shift++;
  const uint64_t per_block = 256u >> g_shift, want = (a->rows_cap + per_block - 1u) / per_block;
  const uint32_t wblocks = (uint32_t)(want < DTK_ENC_MAX_BLOCKS ? (want ? want : 1u) : DTK_ENC_MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  if (blocks) hipLaunchKernelGGL(k_enc_count, dim3(blocks), dim3(DTK_ENC_TILE), 0, s, *a);
  hipLaunchKernelGGL(k_enc_scan, dim3(1), dim3(256), 0, s, *a);
  if (a->word_id) hipLaunchKernelGGL(k_enc_write<true>, dim3(wblocks), dim3(256), 0, s, *a, g_shift);
  else hipLaunchKernelGGL(k_enc_write<false>, dim3(wblocks), dim3(256), 0, s, *a, g_shift);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
