// dtk_streamrender.hip -- the bytes of NewTokenWriter(w, bits) for one slice of a stream (dtk_stream_set_render), in the
// position-free modes: without TOKEN_POS / SENTENCE_POS the writer keeps no state (token_writer.go:91-95, 118-122,
// 162-166), so a slice's bytes are a function of that slice's calls alone.
//
// The calls are the slice's tokens (tok_bstart / tok_bend) merged with its event list (dtk_evlist.hip) by cursor, in
// the order of detail::replay_list (include/datok.hpp); the tail word follows on the stream's last slice.  Sizes:
//   a token under TOKENS        bend - bstart + 2 * (bytes of it that print as U+FFFD) + 1
//   a SentenceEnd call          1 under SENTENCES (SEOT, SEPS, tail S)
//   a TextEnd call              1 (TEOT, tail E)
// Every byte that is no surface byte is '\n': the host fills the output with it, the kernels write surfaces only.
//
// Plain launches on the download stream behind k_evl_*, no block waits for another:
//   k_sr_sums     tiles of 256 tokens, then tiles of 256 list entries: one weight sum per tile
//   k_sr_scan     one block scans both rows of tile sums in place and writes the length word behind the output
//   k_sr_entries  the entry tiles: the exclusive scan of the entry weights, ew[0 .. E]
//   k_sr_copy     the token tiles: a token's offset is its scan value plus ew[] at the lower bound of its end in
//                 evl_pos (plus the SEOT / TEOT part of an entry on the same cursor); a wave then owns 64 consecutive
//                 tokens = one contiguous range of the output, assembles it in LDS in segments of SR_STAGE bytes and
//                 leaves through 16-byte stores of consecutive lanes.  A token part of more than SR_COOP bytes is
//                 copied into the stage by the whole wave.
// With invalid UTF-8 in the run (INV, wave-uniform: a template argument) a lane writes its token byte by byte and
// expands the bytes that did not decode.
// All kernels return at once when the list is longer than its arrays (the host packs it again and renders again), and
// none writes at or behind `cap`.
#include <algorithm>

#include "dtk_device.h"

namespace {

constexpr uint32_t SR_THREADS = 256;
constexpr uint32_t SR_WAVES = SR_THREADS / WAVE;
constexpr uint32_t SR_STAGE = 2048;  // bytes of LDS per wave (a multiple of 16 * WAVE)
constexpr uint32_t SR_COOP = 64;     // a longer part of a token goes into the stage by the whole wave
static_assert(SR_STAGE % (16u * WAVE) == 0u, "the fill and the flush take whole rounds of the wave");

struct SrTok { uint32_t bs, len; uint64_t w; };

// token k: first byte, surface bytes in the text, bytes in the output (0 behind the last token)
template <bool INV>
__device__ __forceinline__ SrTok sr_token(const DtkStreamRenderArgs &A, uint64_t k) {
  SrTok t{0u, 0u, 0u};
  if (k >= A.n_tok) return t;
  const uint32_t bs = A.tok_bstart[k], be = A.tok_bend[k];
  t.bs = bs;
  t.len = (be > bs && be <= A.text_len) ? be - bs : 0u;  // (start > end: DTK_ST_BAD_OFFSET, out of contract)
  t.w = (uint64_t)t.len + 1u;
  if (INV) t.w += 2u * sym_invalid_count(A.sym, bs, t.len);
  return t;
}

// entry j: bytes in front of a token on its cursor (SEOT, TEOT) and behind it (SEPS)
__device__ __forceinline__ void sr_entry(const DtkStreamRenderArgs &A, uint32_t kind, uint32_t &pre, uint32_t &post) {
  const uint32_t s = (A.bits >> 1) & 1u;
  pre = ((kind & DTK_EVL_K_SEOT) ? s : 0u) + ((kind & DTK_EVL_K_TEOT) ? 1u : 0u);
  post = (kind & DTK_EVL_K_SEPS) ? s : 0u;
}

template <bool INV>
__global__ __launch_bounds__(256) void k_sr_sums(DtkStreamRenderArgs A) {
  __shared__ uint64_t wave_tot[SR_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;  // (block-uniform)
  uint64_t w = 0;
  const bool tok = blockIdx.x < A.tok_tiles;
  if (tok) {
    if (A.bits & 1u) w = sr_token<INV>(A, (uint64_t)blockIdx.x * SR_THREADS + threadIdx.x).w;
  } else {
    const uint32_t j = (blockIdx.x - A.tok_tiles) * SR_THREADS + threadIdx.x;
    if (j < E) {
      uint32_t pre, post;
      sr_entry(A, A.evl_kind[j], pre, post);
      w = pre + post;
    }
  }
  uint64_t total;
  (void)block_excl_scan64(w, wave_tot, total);
  if (threadIdx.x == 0u) (tok ? A.tok_base[blockIdx.x] : A.ent_base[blockIdx.x - A.tok_tiles]) = total;
}

__global__ __launch_bounds__(256) void k_sr_scan(DtkStreamRenderArgs A) {
  __shared__ uint64_t wave_tot[SR_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) {
    if (threadIdx.x == 0u) *A.out_len = ~0ull;
    return;
  }
  uint64_t sum[2];
  for (uint32_t r = 0; r < 2u; r++) sum[r] = scan_row64(r ? A.ent_base : A.tok_base, r ? A.ent_tiles : A.tok_tiles, wave_tot);
  if (threadIdx.x != 0u) return;
  A.ew[E] = sum[1];
  uint64_t tail = 0;
  if (A.with_tail) {
    const uint32_t t = A.doc_tail[0];
    tail = ((t & DTK_TAIL_S) ? ((A.bits >> 1) & 1u) : 0u) + ((t & DTK_TAIL_E) ? 1u : 0u);
  }
  *A.out_len = sum[0] + sum[1] + tail;
}

__global__ __launch_bounds__(256) void k_sr_entries(DtkStreamRenderArgs A) {
  __shared__ uint64_t wave_tot[SR_WAVES];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint32_t j = blockIdx.x * SR_THREADS + threadIdx.x;
  uint32_t pre = 0, post = 0;
  if (j < E) sr_entry(A, A.evl_kind[j], pre, post);
  uint64_t total;
  const uint64_t x = block_excl_scan64((uint64_t)pre + post, wave_tot, total);
  if (j < E) A.ew[j] = A.ent_base[blockIdx.x] + x;
}

template <bool INV>
__global__ __launch_bounds__(256) void k_sr_copy(DtkStreamRenderArgs A) {
  __shared__ uint64_t wave_tot[SR_WAVES];
  __shared__ __attribute__((aligned(16))) uint8_t stage_all[SR_WAVES][SR_STAGE];
  const uint32_t E = evl_entries(A);
  if (E == 0xFFFFFFFFu) return;
  const uint64_t k = (uint64_t)blockIdx.x * SR_THREADS + threadIdx.x;
  const SrTok t = sr_token<INV>(A, k);
  uint64_t total;
  uint64_t off = A.tok_base[blockIdx.x] + block_excl_scan64(t.w, wave_tot, total);
  const bool valid = k < A.n_tok;
  if (valid) {
    // the entries in front of the token: the first entry at or behind its end
    const uint32_t be = A.tok_bend[k];
    const uint32_t lo = lower_bound32(A.evl_pos, E, be);
    off += A.ew[lo];
    if (lo < E && A.evl_pos[lo] == be) {
      uint32_t pre, post;
      sr_entry(A, A.evl_kind[lo], pre, post);
      off += pre;
    }
  }
  const uint8_t *__restrict__ text = A.text;
  uint8_t *__restrict__ out = A.out;
  if (INV) {
    if (valid) sym_expand(A.sym, text, t.bs, t.len, out, off, A.cap);
    return;
  }
  // ---- the wave's 64 tokens: the output range [base, base + range), staged from its 16-byte boundary `abase` on
  if (!__builtin_amdgcn_readfirstlane((int)valid)) return;  // (lane 0 has no token: none of the wave has)
  uint8_t *stage = stage_all[threadIdx.x >> 6];
  const uint32_t lane = lane_id();
  const uint32_t lo32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)off);
  const uint32_t hi32 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(off >> 32));
  const uint64_t base = ((uint64_t)hi32 << 32) | lo32;
  const uint64_t abase = base & ~15ull;
  if (abase >= A.cap) return;
  const uint64_t room = A.cap - abase;
  const uint32_t cap_rel = room > 0x7FFFFFF0ull ? 0x7FFFFFF0u : (uint32_t)room;
  const uint32_t base_rel = (uint32_t)(base - abase);
  // (64 tokens of one window and the newlines between them: far below 2^31)
  const uint64_t rel64 = off - abase;
  const bool sane = valid && rel64 < 0x40000000ull && t.len < 0x20000000u;
  const uint32_t rel = sane ? (uint32_t)rel64 : 0u;
  const uint32_t len = sane ? t.len : 0u;
  const uint32_t range_end = std::min((uint32_t)wave_max(sane ? (int32_t)(rel + len + 1u) : 0), cap_rel);
  for (uint32_t seg0 = 0; seg0 < range_end; seg0 += SR_STAGE) {  // (wave-uniform)
    const uint32_t seg1 = std::min(seg0 + SR_STAGE, range_end);
    const uint4 nl = make_uint4(0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au, 0x0A0A0A0Au);
#pragma unroll
    for (uint32_t u = 0; u < SR_STAGE / (16u * WAVE); u++) reinterpret_cast<uint4 *>(stage)[u * WAVE + lane] = nl;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the part of the lane's surface that lies in this segment
    const uint32_t a = std::max(rel, seg0), z = std::min(rel + len, seg1);
    const uint32_t n = z > a ? z - a : 0u;
    const uint32_t src = t.bs + (a - rel);
    if (n <= SR_COOP)
      for (uint32_t q = 0; q < n; q++) stage[a - seg0 + q] = text[src + q];
    unsigned long long coop = __ballot(n > SR_COOP);
    while (coop) {  // (wave-uniform)
      const int l = __builtin_ctzll(coop);
      coop &= coop - 1ull;
      const uint32_t a_l = (uint32_t)__shfl((int)a, l), n_l = (uint32_t)__shfl((int)n, l), src_l = (uint32_t)__shfl((int)src, l);
      for (uint32_t q = lane; q < n_l; q += WAVE) stage[a_l - seg0 + q] = text[src_l + q];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // out: whole 16-byte units of consecutive lanes; the range's first and last unit byte by byte
    for (uint32_t u0 = seg0 + lane * 16u; u0 < seg1; u0 += WAVE * 16u) {
      const uint32_t w0 = std::max(u0, base_rel), w1 = std::min(u0 + 16u, seg1);
      if (w0 == u0 && w1 == u0 + 16u) {
        *reinterpret_cast<uint4 *>(out + abase + u0) = *reinterpret_cast<const uint4 *>(stage + (u0 - seg0));
      } else {
        for (uint32_t q = w0; q < w1; q++) out[abase + q] = stage[q - seg0];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

extern "C" uint32_t dtk_streamrender_tiles(uint64_t n) { return (uint32_t)((n + SR_THREADS - 1u) / SR_THREADS); }

extern "C" int dtk_launch_streamrender(const DtkStreamRenderArgs *args, void *stream) {
  DtkStreamRenderArgs A = *args;
  hipStream_t s = (hipStream_t)stream;
  if (A.n_tok > 0xFFFFFFFFull * SR_THREADS || A.tok_tiles != dtk_streamrender_tiles(A.n_tok) ||
      A.ent_tiles != dtk_streamrender_tiles(A.evl_cap) || (A.bits & ~3u) || ((uintptr_t)A.out & 15u))
    return 1;
  const bool inv = A.sym.base != nullptr;
  const bool surfaces = (A.bits & 1u) && A.tok_tiles;
  const uint32_t sum_tiles = (surfaces ? A.tok_tiles : 0u) + A.ent_tiles;
  if (!surfaces) A.tok_tiles = 0;  // (no token has a byte: the entries and the tail are the output)
  if (sum_tiles) {
    if (inv) hipLaunchKernelGGL(k_sr_sums<true>, dim3(sum_tiles), dim3(SR_THREADS), 0, s, A);
    else hipLaunchKernelGGL(k_sr_sums<false>, dim3(sum_tiles), dim3(SR_THREADS), 0, s, A);
  }
  hipLaunchKernelGGL(k_sr_scan, dim3(1), dim3(SR_THREADS), 0, s, A);
  if (A.ent_tiles) hipLaunchKernelGGL(k_sr_entries, dim3(A.ent_tiles), dim3(SR_THREADS), 0, s, A);
  if (surfaces) {
    if (inv) hipLaunchKernelGGL(k_sr_copy<true>, dim3(A.tok_tiles), dim3(SR_THREADS), 0, s, A);
    else hipLaunchKernelGGL(k_sr_copy<false>, dim3(A.tok_tiles), dim3(SR_THREADS), 0, s, A);
  }
  return (int)hipGetLastError();
}
