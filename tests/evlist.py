"""The event list of a closure replay (DTK_R_EVENT_LIST), in plain numpy (test infrastructure).

Written from the definition in include/datok_gpu.h, not from the kernels: it is the CPU-side definition that the
kernels of dtk_evlist.hip and the replays (datok_amd.replay_list, detail::replay_list) are compared against.

    document d has one entry for every cursor p in 0..len(d) at which bit  doc_off[d] + d + p  is set in any of the
    bitmaps SEPS, TEOT, SEOT;  evl_kind says in which of them:  SEOT 1, TEOT 2, SEPS 4
    evl_off[d] .. evl_off[d + 1] are the entries of document d;  evl_pos is document relative and ascending
"""
import numpy as np

EVB_SEPS, EVB_TEOT, EVB_SEOT = 2, 3, 4                       # datok_gpu.h DTK_EVB_*
EVL_SEOT, EVL_TEOT, EVL_SEPS = 1, 2, 4                       # datok_gpu.h DTK_EVL_*
EV_S_EOT, EV_E_EOT, EV_TOK_END, EV_S_EPS, EV_S_EPS2, EV_S_EOF, EV_E_EOF = 1, 2, 4, 8, 16, 32, 64   # test_host_logic.py


# ---- part 1: from the bitmaps and the document offsets
def from_bitmaps(ev_bits, doc_off):
    """(evl_off uint32[n_docs + 1], evl_pos uint32[n], evl_kind uint8[n], global bit of every entry) from the event
    bitmaps of a host result (uint32[5, words]) and the batch's document offsets."""
    doc_off = np.asarray(doc_off).astype(np.int64)
    n_docs = len(doc_off) - 1
    bit0 = doc_off + np.arange(n_docs + 1)                  # bit of position 0 of document d; [n_docs]: the end
    n_bits = int(bit0[-1])

    def bits(kind):     # (bits at or behind n_bits belong to no document)
        return np.unpackbits(np.ascontiguousarray(ev_bits[kind]).view(np.uint8), bitorder="little")[:n_bits]
    seps, teot, seot = bits(EVB_SEPS), bits(EVB_TEOT), bits(EVB_SEOT)
    g = np.flatnonzero(seps | teot | seot)
    d = np.searchsorted(bit0[:n_docs], g, side="right") - 1
    pos = g - bit0[d]
    assert (pos >= 0).all() and (pos <= doc_off[d + 1] - doc_off[d]).all()
    kind = seot[g] * EVL_SEOT | teot[g] * EVL_TEOT | seps[g] * EVL_SEPS
    off = np.searchsorted(g, bit0, side="left")
    return off.astype(np.uint32), pos.astype(np.uint32), kind.astype(np.uint8), g


# ---- part 2: from the event bytes of tests/test_host_logic.py::matrix_events (the oracle's calls of one document)
def from_event_bytes(ev):
    """(evl_pos, evl_kind, tail word, END cursors) of one document.  A second epsilon SentenceEnd at one cursor has no
    place in the bitmaps (such a document goes to the exact pass): refused here."""
    ev = np.asarray(ev)
    assert not (ev & EV_S_EPS2).any()
    listed = ev & (EV_S_EOT | EV_E_EOT | EV_S_EPS)
    pos = np.flatnonzero(listed)
    e = ev[pos]
    kind = ((e & EV_S_EOT) != 0) * EVL_SEOT | ((e & EV_E_EOT) != 0) * EVL_TEOT | ((e & EV_S_EPS) != 0) * EVL_SEPS
    at = np.flatnonzero(ev & (EV_S_EOF | EV_E_EOF))
    assert len(at) <= 1
    tail = 0
    if len(at):
        p = int(at[0])
        tail = p << 2 | (1 if ev[p] & EV_S_EOF else 0) | (2 if ev[p] & EV_E_EOF else 0)
    return pos.astype(np.uint32), kind.astype(np.uint8), tail, np.flatnonzero(ev & EV_TOK_END).astype(np.uint32)


# ---- part 3: a recording TokenWriter, and the oracle's calls in the same form
class Recorder:
    """A custom TokenWriter (token_writer.go:27-33): logs every call with its arguments."""

    def __init__(self):
        self.calls = []
        self.Token = lambda off, buf: self.calls.append(("T", off, len(buf)))
        self.SentenceEnd = lambda a: self.calls.append(("S", a))
        self.TextEnd = lambda a: self.calls.append(("E", a))
        self.Flush = lambda: None


def oracle_calls(om, doc: bytes):
    """[('T', offset, len(buf)) | ('S', arg) | ('E', arg)] in the reference's call order (oracle.Model.events())."""
    from datok_amd.host import _decode_runes
    out = []
    for kind, a, b, c, d in om.events(doc)[0]:
        out.append(("T", a, len(_decode_runes(doc[b:d])) if d > b else 0) if kind == 0 else ("SE"[kind - 1], a))
    return out


def replayed(res, d, doc: bytes, is_matrix):
    """The call log of document d of a BatchResult: from `calls` if the exact pass walked it, else from the list."""
    from datok_amd import host
    rec = Recorder()
    if d in res.exact:
        host.replay_calls(doc, res.exact[d], rec)
    else:
        row = res.doc(d)
        host.replay_list(is_matrix, doc, row["evl_pos"], row["evl_kind"], res.doc_tail[d], row["tok_bstart"], row["tok_bend"], rec)
    return rec.calls
