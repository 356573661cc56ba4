// dtk_streamcut.hip -- a slice of one long stream (dtk_stream_run): ends the slice's document
// at its cut.  The slice's window [0, S + T) was walked as one document; the start record of the first lane that begins
// at or behind S is verified like every other (k_spec_verify) and lies below S + DTK_WINDOW_BYTES, so nothing the walk
// did in front of it has seen the window's false end.  Everything at or behind that record is the next slice's.
//
// One block, enqueued between the verification (and the device-side repair rounds) and the scan; like the scan and the
// compaction it does nothing while documents are still to repair (finish() then runs it behind the host's rounds).
#include "dtk_device.h"

#define CUT_TB 1024u

__global__ __launch_bounds__(CUT_TB) void k_stream_cut(DtkStreamCutArgs X) {
  if (X.skip_if && *X.skip_if != 0u) return;
  __shared__ uint32_t s_sum[3], s_front;
  if (threadIdx.x < 3u) s_sum[threadIdx.x] = 0u;
  if (threadIdx.x == 3u) s_front = 0u;
  __syncthreads();
  const uint32_t tid = threadIdx.x;
  // the lane that walked from the carried record: the last one whose chunk does not begin behind it
  const bool carried = X.init_rec != nullptr;
  uint32_t walker = 0xFFFFFFFFu, walker_st = 0u, walker_end = 0xFFFFFFFFu;
  if (carried && X.chunk != 0u) {
    walker = X.init_rec[0].p / X.chunk;
    if (walker >= X.n_lanes) walker = X.n_lanes - 1u;
    walker_st = X.lane_cnt[walker].status;
    if (walker + 1u < X.n_lanes) walker_end = X.lane_start[walker + 1u].p;
  }
  // the cut: the record of the first lane that begins at or behind S
  const uint32_t lc = X.chunk ? (X.slice + X.chunk - 1u) / X.chunk : 0u;
  DtkLaneState rec{0xFFFFFFFFu, 0u, 0u, 0u};
  if (X.slice) {
    if (X.chunk == 0u) rec = X.open_fin[0];
    else if (lc < X.n_lanes) rec = X.lane_start[lc];
  }
  const bool cut = rec.p != 0xFFFFFFFFu;
  const uint32_t front = X.chunk ? (cut ? lc : X.n_lanes) : 0u;  // lanes whose reports stay
  if (X.chunk != 0u) {
    // the document's walk status from the lanes in front of the cut alone (a lane behind it may have raised any bit
    // against the window's false end), without the lane that walked from the carried record
    // (a lane without a record lies behind the chain's end: the verification did not count it either)
    uint32_t st = 0u;
    for (uint32_t L = tid; L < front; L += CUT_TB)
      if (L != walker && X.lane_start[L].p != 0xFFFFFFFFu) st |= X.lane_cnt[L].status;
    if (st) atomicOr(&s_front, st);
    if (cut) {
      // what the lanes behind the cut counted leaves the document's counters, and their own: the scan, the segment
      // sums and the compaction's check sum see a document that ends at the cut
      uint32_t tok = 0u, sent = 0u, text = 0u;
      for (uint32_t L = lc + tid; L < X.n_lanes; L += CUT_TB) {
        const DtkLaneCount c = X.lane_cnt[L];
        if (X.lane_start[L].p != 0xFFFFFFFFu) { tok += c.tok; sent += c.sent; text += c.text; }
        X.lane_cnt[L] = DtkLaneCount{0u, 0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0u};
      }
      if (tok) atomicAdd(&s_sum[0], tok);
      if (sent) atomicAdd(&s_sum[1], sent);
      if (text) atomicAdd(&s_sum[2], text);
    }
  }
  if (cut) {
    // Every bit behind the cut goes; at the cut itself only the opening kinds do (k_redo_clear's rule): the closing
    // kinds there were reported by the lane that stopped at it.  (One document at offset 0: position p is bit p.)
    for (uint32_t j = (rec.p >> 5) + tid; j < X.bit_words; j += CUT_TB) {
      const uint64_t g0 = 32ull * j;
      uint32_t m_all = 0xFFFFFFFFu, m_open = 0xFFFFFFFFu;
      if (g0 <= rec.p) {
        const uint32_t sh = rec.p - (uint32_t)g0;  // 0..31
        m_open = 0xFFFFFFFFu << sh;
        m_all = sh == 31u ? 0u : 0xFFFFFFFFu << (sh + 1u);
      }
      if (m_all) {
        X.bits[EVB_END * X.bit_words + j] &= ~m_all;
        X.bits[EVB_TEOT * X.bit_words + j] &= ~m_all;
        X.bits[EVB_SEOT * X.bit_words + j] &= ~m_all;
      }
      X.bits[EVB_START * X.bit_words + j] &= ~m_open;
      X.bits[EVB_SEPS * X.bit_words + j] &= ~m_open;
    }
  }
  __syncthreads();
  if (tid != 0u) return;
  if (X.chunk != 0u) {
    X.status[0] = s_front;
    if (cut) {
      X.tok_cnt[0] -= s_sum[0]; X.sent_cnt[0] -= s_sum[1]; X.text_cnt[0] -= s_sum[2];
    }
  } else if (carried) {
    // one lane for the whole document: it is the lane that walked from the carried record
    walker_st = X.status[0];
    X.status[0] = 0u;
  }
  if (cut) X.doc_tail[0] = 0u;
  DtkStreamCut o;
  o.p = cut ? rec.p - X.slice : 0xFFFFFFFFu; o.t = rec.t; o.aux = rec.aux;
  o.flags = rec.flags & (LANE_F_SENT | LANE_F_TEXT | LANE_F_OK);
  o.cut = rec.p;
  o.valid = 1u;
  o.walker_status = walker_st; o.walker_end = walker_end;
  *X.out = o;
}

extern "C" int dtk_launch_stream_cut(const DtkStreamCutArgs *args, void *stream) {
  hipLaunchKernelGGL(k_stream_cut, dim3(1), dim3(CUT_TB), 0, (hipStream_t)stream, *args);
  return (int)hipGetLastError();
}
