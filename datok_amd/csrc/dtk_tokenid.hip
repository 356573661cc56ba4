// dtk_tokenid.hip -- every token of a finished run looked up in a vocabulary (dtk_batch_set_vocab, include/datok_gpu.h):
// tok_id[i] is the index of the word equal to token i's key -- the surface as the reference's writer prints it,
// string(buf[offset:]) (token_writer.go:85,93): the document's bytes [tok_bstart, tok_bend) with every byte that does
// not decode replaced by EF BF BD -- or -1.  One lane per token: it finds its document, hashes the key, probes the
// table (dtk_vocab_core.h, the code the builder and the host probe use) and compares the bytes.  Runs on the download
// stream behind finish(), so the token count is final and repairs and the exact pass are done.
//
// A run without invalid UTF-8 never touches the symbol stream: its keys are the text's bytes, read as aligned 32-bit
// words (the last word read is the one that holds the key's last byte).  With invalid bytes in the run the key is
// produced a byte at a time under the renderers' rule (sym_invalid_byte).  Both key types live in dtk_key.h, which the
// WordPiece kernels (dtk_wordpiece.hip) share.  With a fold attached (dtk_batch_set_fold) the key is F(K): either key type
// read through FoldedKey, rune by rune, with the fold's ASCII page in LDS.
//
// Counts: the unknowns of a wave go to the batch's counter with one atomic per wave.  With a tally attached every
// token adds 1 to its id's 64-bit counter.  Natural text is Zipfian and vocabularies come sorted by frequency, so the
// ids below DTK_TALLY_HOT are counted in LDS first and a block adds its non-zero counters once at its end; the others
// go straight to global atomics, where they are spread over many addresses.  Integer adds only: the counts are exact
// in any order.
#include <hip/hip_runtime.h>

#include "dtk_internal.h"
#include "dtk_vocab_core.h"
#include "dtk_device.h"
#include "dtk_key.h"

#define DTK_TOKID_THREADS 256u
#define DTK_TOKID_MAX_BLOCKS 2048u
#define DTK_TALLY_HOT 2048u  // ids counted in LDS (8 KiB of 32-bit counters per block)

namespace {
template <class Key>
__device__ __forceinline__ int32_t lookup(const DtkVocabDev &V, const Key &key) {
  uint32_t len;
  const uint64_t h = key.hash(V.hash_bits, &len);
  return dtk_vocab_find(
      V, h,
      [&](uint32_t w) {
        const uint32_t o = V.off[w];
        return V.off[w + 1u] - o == len && key.equals(V.bytes + o, len);
      },
      nullptr);
}

// FOLD: the launch has a fold attached (dtk_batch_set_fold) and every key is read through it; chosen per launch, so
// the kernel of a run without a fold is the one it was.
template <bool FOLD>
__global__ __launch_bounds__(DTK_TOKID_THREADS) void k_token_ids(const DtkTokenIdArgs a) {
  __shared__ uint32_t hot[DTK_TALLY_HOT];
  __shared__ uint32_t fold_ascii[FOLD ? DTK_FOLD_PAGE : 1u];
  if constexpr (FOLD) stage_fold_ascii(a.fold, fold_ascii);
  const bool tally = a.tally != nullptr;
  if (tally) {
    for (uint32_t j = threadIdx.x; j < DTK_TALLY_HOT; j += DTK_TOKID_THREADS) hot[j] = 0u;
    __syncthreads();
  }
  const DtkSym S{a.sym_base, a.sym_lut};
  // (the loop's bounds are the block's: every lane of a wave takes part in the ballot below)
  for (uint64_t t0 = (uint64_t)blockIdx.x * DTK_TOKID_THREADS; t0 < a.n_tok; t0 += (uint64_t)gridDim.x * DTK_TOKID_THREADS) {
    const uint64_t i = t0 + threadIdx.x;
    const bool live = i < a.n_tok;
    int32_t id = -1;
    if (live) {
      // The token's document: the last d with tok_off[d] <= i (documents without a token have equal neighbours).  A
      // search per token: a variant that searched once per thread and stepped from there measured the same
      // (136.4 against 137.4 us on the bench batch), so the plain form stays.
      uint32_t lo = 0, hi = a.n_docs;
      while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.tok_off[mid] <= i) lo = mid; else hi = mid;
      }
      const uint64_t d0 = a.doc_off[lo], d1 = a.doc_off[lo + 1u];
      const uint64_t len = d1 > d0 && d1 <= a.total ? d1 - d0 : 0u;
      uint64_t bs = a.tok_bstart[i], be = a.tok_bend[i];
      if (bs <= be) {  // (start > end: a Token call the reference cannot print, DTK_ST_BAD_OFFSET)
        // rows of flagged documents are clamped to the document: nothing outside its bytes is read
        if (be > len) be = len;
        if (bs > be) bs = be;
        const uint8_t *p = a.text + d0 + bs;
        const uint32_t n = (uint32_t)(be - bs);
        if constexpr (FOLD) {
          id = a.sym_base ? lookup(a.vocab, FoldedKey<ReplacedKey>{ReplacedKey{p, n, S, d0 + bs}, a.fold, fold_ascii})
                          : lookup(a.vocab, FoldedKey<RawKey>{RawKey{p, n}, a.fold, fold_ascii});
        } else {
          id = a.sym_base ? lookup(a.vocab, ReplacedKey{p, n, S, d0 + bs}) : lookup(a.vocab, RawKey{p, n});
        }
      }
      a.tok_id[i] = id;
    }
    const uint32_t unknown = (uint32_t)__popcll(__ballot(live && id < 0));
    if ((threadIdx.x & 63u) == 0u && unknown) {
      atomicAdd(a.n_unknown, (unsigned long long)unknown);
      if (tally) atomicAdd(a.tally + a.vocab.n_words, (unsigned long long)unknown);
    }
    if (tally && id >= 0) {
      if ((uint32_t)id < DTK_TALLY_HOT) atomicAdd(&hot[id], 1u);
      else atomicAdd(a.tally + id, 1ull);
    }
  }
  if (tally) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < DTK_TALLY_HOT; j += DTK_TOKID_THREADS) {
      const uint32_t c = hot[j];
      if (c) atomicAdd(a.tally + j, (unsigned long long)c);  // (c != 0: j is an id some token got, so j < n_words)
    }
  }
}
}  // namespace

extern "C" int dtk_launch_token_ids(const DtkTokenIdArgs *a, void *stream) {
  if (a->n_tok == 0) return 0;
  const uint64_t tiles = (a->n_tok + DTK_TOKID_THREADS - 1u) / DTK_TOKID_THREADS;
  const uint32_t blocks = (uint32_t)(tiles < DTK_TOKID_MAX_BLOCKS ? tiles : DTK_TOKID_MAX_BLOCKS);
  if (a->fold.entry) hipLaunchKernelGGL(k_token_ids<true>, dim3(blocks), dim3(DTK_TOKID_THREADS), 0, (hipStream_t)stream, *a);
  else hipLaunchKernelGGL(k_token_ids<false>, dim3(blocks), dim3(DTK_TOKID_THREADS), 0, (hipStream_t)stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
