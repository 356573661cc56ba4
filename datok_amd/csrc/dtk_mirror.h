// dtk_mirror.h -- a block in device memory and its page-locked copy, of one byte layout that is fixed before anything is
// enqueued: the tables a download computes on its stream and brings home (a slice's bytes, offsets and sentence rows,
// dtk_slice.cpp; the batch's sentence table, dtk_results.cpp).  The first copies are sized by a bound the host can state
// early; a trailer or count word in the block says whether the bound held, and what is missing comes at delivery.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#pragma GCC visibility push(hidden)

// A piece of a block: T is its element type, stated where the handle is declared -- the pointers into both blocks and
// every byte count follow from it.
template <class T>
struct Piece { uint32_t i = 0; };

// The layout (no HIP call: it compiles on its own, with DTK_MIRROR_LAYOUT_ONLY defined).  Pieces are added in order; each
// begins on a multiple of 8 bytes, and one of no element takes no room.
struct MirrorLayout {
  struct Part { uint64_t at, size, cap, home; };  // byte offset, element size; elements: capacity, held by the page-locked copy
  struct Range { uint64_t from, to; };            // bytes
  std::vector<Part> parts;
  std::vector<Range> pending;   // what bring() has asked for and nobody has copied yet
  uint64_t bytes = 0;           // of the block
  uint64_t joins_at = ~0ull;    // the last range reaches its piece's end: where the next piece begins, padding included

  void clear() { parts.clear(); pending.clear(); bytes = 0; joins_at = ~0ull; }
  template <class T> void add(Piece<T> &p, uint64_t cap) {
    p.i = (uint32_t)parts.size();
    parts.push_back(Part{bytes, sizeof(T), cap, 0});
    bytes += (cap * sizeof(T) + 7u) & ~7ull;
  }
  template <class T> uint64_t at(Piece<T> p) const { return parts[p.i].at; }
  template <class T> uint64_t cap(Piece<T> p) const { return parts[p.i].cap; }
  template <class T> uint64_t home(Piece<T> p) const { return parts[p.i].home; }
  template <class T> T *in(void *block, Piece<T> p) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(block) + parts[p.i].at); }
  // The page-locked copy shall hold the piece's first n elements (at most its capacity): the missing ones join the
  // pending ranges.  A range that begins a piece goes into the one that ended the piece in front of it (the padding
  // between them is copied too).
  template <class T> void bring(Piece<T> p, uint64_t n) {
    Part &q = parts[p.i];
    n = std::min(n, q.cap);
    if (n <= q.home) return;
    const uint64_t from = q.at + q.home * q.size, to = q.at + n * q.size;
    if (!pending.empty() && (from == pending.back().to || from == joins_at)) pending.back().to = to;
    else pending.push_back(Range{from, to});
    joins_at = n == q.cap ? q.at + ((q.cap * q.size + 7u) & ~7ull) : ~0ull;
    q.home = n;
  }
};

#ifndef DTK_MIRROR_LAYOUT_ONLY
#include "dtk_own.h"

// The two blocks of a layout.  The host side is optional: a block whose results only kernels read brings nothing home.
struct MirrorBlock : MirrorLayout, NoCopy {
  DevArray<uint64_t> d;
  PinBuf h;
  bool in_flight = false;  // copies have been issued that nobody has waited for (landed())

  int fit(bool host = true) {  // room for the layout as it stands; contents are lost where a block grows
    const uint64_t words = bytes / 8;
    const int rc = d.fit(words, words + words / 8 + 32);
    return rc != DTK_OK || !host ? rc : h.fit((size_t)bytes);
  }
  template <class T> T *dev(Piece<T> p) const { return in(d.p, p); }
  template <class T> T *host(Piece<T> p) const { return in(h.p, p); }
  // the pending ranges, one copy each
  int issue(hipStream_t s) {
    for (const Range &r : pending) {
      HIP_TRY(hipMemcpyAsync(h.as<uint8_t>() + r.from, reinterpret_cast<const uint8_t *>(d.p) + r.from, (size_t)(r.to - r.from),
                             hipMemcpyDeviceToHost, s));
      in_flight = true;
    }
    pending.clear();
    return DTK_OK;
  }
  void landed() { in_flight = false; }  // the caller has waited for the stream, or for an event behind the copies
};
#endif

#pragma GCC visibility pop
