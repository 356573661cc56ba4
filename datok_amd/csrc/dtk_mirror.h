// dtk_mirror.h -- a block in device memory and its page-locked copy, of one byte layout that is fixed before anything is
// enqueued: the tables a download computes on its stream and brings home (a slice's bytes, offsets and sentence rows,
// dtk_slice.cpp; the batch's derived tables, dtk_derived.cpp).  The first copies are sized by a bound the host can state
// early; a trailer or count word in the block says whether the bound held, and what is missing comes at delivery.
#pragma once
#include <stdint.h>

#include "../../include/datok_gpu.h"

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
  void all_home() {  // the host has written the page-locked copy itself: nothing is missing, nothing is asked for
    for (Part &q : parts) q.home = q.cap;
    pending.clear();
  }
};

// The state of a derived table, the part without a HIP call: a table that is computed once per
// run into a block sized by a bound, with a count word that says whether the bound held.
struct DerivedState {
  bool built = false;  // the kernels have been enqueued for this run, into the block as it is described
  uint32_t gen = 0;    // counts launches and rewrites: what is computed from the table knows which state it read
  uint64_t need = 0;   // nonzero: a run had that many elements, more than the bound
  void launched() { built = true; gen++; }
  void new_run(bool keep_need = false) { built = false; if (!keep_need) need = 0; }
};

// What a table computed from two others read of them: stale exactly when either has moved since.
struct DerivedReads {
  uint32_t a = 0, b = 0;
  bool stale(uint32_t a_now, uint32_t b_now) const { return a != a_now || b != b_now; }
};

// Completes a table.  step(): enqueues what is missing and waits for it; fits(n): the count as it came home -- true, or n
// elements are needed and nothing was written.  Then once more, into a block of that size: a run's count cannot grow, so a
// second overflow is an error.
template <class Step, class Fits>
int derived_complete(DerivedState &s, Step step, Fits fits) {
  for (int round = 0;; round++) {
    const int rc = step();
    if (rc != DTK_OK) return rc;
    uint64_t n = 0;
    if (fits(n)) return DTK_OK;
    if (round) return DTK_E_STATE;
    s.need = n;
    s.built = false;
  }
}

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

// A derived table: its blocks, its state, and the event behind what was last enqueued for it.  Nobody touches the
// table's inputs or its blocks before wait().
struct DerivedBlock : MirrorBlock, DerivedState {
  Event ev;
  bool waited = true;  // ev has been waited for: what was enqueued is there
  // Copies the pending ranges and records behind them and behind what the caller has just enqueued (`launched`: kernels
  // that asked for no copy).  Nothing of either: no HIP call.
  int record(hipStream_t s, bool launched = false) {
    if (pending.empty() && !launched) return DTK_OK;
    int rc;
    if ((rc = issue(s)) != DTK_OK || (rc = ev.ensure(hipEventDisableTiming)) != DTK_OK) return rc;
    HIP_TRY(hipEventRecord(ev, s));
    waited = false;
    return DTK_OK;
  }
  int wait() {
    if (waited) return DTK_OK;
    HIP_TRY(hipEventSynchronize(ev));
    waited = true;
    landed();
    return DTK_OK;
  }
};
#endif

#pragma GCC visibility pop
