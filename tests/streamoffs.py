"""The reference of a stream's offset delivery (test infrastructure): tests/test_stream_offsets_host.py,
tests/test_stream_offsets.py.

offsets_slice_ref states in plain Python what dtk_streamoffs.hip computes for one slice of a stream: the integers a
NewTokenWriter with TOKEN_POS | SENTENCE_POS collects in pos[] and sent[] (token_writer.go:36-175) during the slice's
calls -- the tokens merged with the event list by cursor, as streampos.render_slice_pos_ref merges them -- from the state
that crossed the cut, with the C++ mirror's and the oracle's answer to an empty text (the push is skipped).
pack_blocked64_ref / unpack_blocked64_ref are dtk_off_block64 (include/datok_gpu.h) in numpy.
"""
import numpy as np

from datok_amd.host import EVL_SEOT, EVL_SEPS, EVL_TEOT, _decode_runes

HEAD64 = np.dtype([("base0", np.int64), ("base1", np.int64), ("brk", np.uint32), ("reserved", np.uint32)])
SPAN = 65535


def offsets_slice_ref(is_matrix, sl, nl, carry_in):
    """(rstart, rend, sent, text_tok_end, text_sent_end, carry_out) of the slice `sl` (a SliceView) for a writer that
    enters it in the state carry_in = (posC, sentB, init, pos non-empty, sent non-empty).  rstart / rend / sent: int64
    arrays; text_tok_end / text_sent_end: tokens / sent ints of THIS slice in front of each TextEnd call."""
    posC, sentB, init, pne, sne = carry_in
    text, n = sl.text, len(sl.text)
    rstart, rend, sent, tte, tse = [], [], [], [], []

    def runes(a, z):
        return len(_decode_runes(text[a:z]))

    def sentence_end():
        nonlocal sentB, sne
        if pne:
            sent.append(posC)              # pos.back() == posC
            sne = True
        sentB = True

    def text_end():
        nonlocal posC, pne, sne, sentB
        tte.append(len(rstart))
        tse.append(len(sent))
        sne, sentB = False, True
        posC, pne = 0, False

    B = int(sl.first)
    k = j = 0
    nt, ne = len(sl.tok_bend), len(sl.evl_pos)
    while k < nt or j < ne:
        pt = int(sl.tok_bend[k]) if k < nt else n + 1
        pe = int(sl.evl_pos[j]) if j < ne else n + 1
        p = min(pt, pe)
        e = 0
        if pe == p:
            e = int(sl.evl_kind[j])
            j += 1
        if e & EVL_SEOT:
            sentence_end()
        if e & EVL_TEOT:
            text_end()
            if is_matrix:
                B = p
        if pt == p:
            start = int(sl.tok_bstart[k])
            k += 1
            if posC == 0 and nl and B < n and text[B] == 10 and not init:
                posC -= 1
            init = False
            posC += runes(B, start)
            rstart.append(posC)
            pne = True
            if sentB:
                sentB = False
                sent.append(posC)
                sne = True
            posC += runes(start, p)
            rend.append(posC)
            B = p
        if e & EVL_SEPS:
            sentence_end()
    if sl.last:
        if int(sl.tail) & 1:
            sentence_end()
        if int(sl.tail) & 2:
            text_end()
    return (np.array(rstart, np.int64), np.array(rend, np.int64), np.array(sent, np.int64), np.array(tte, np.uint32),
            np.array(tse, np.uint32), (posC, sentB, init, pne, sne))


def join_slices(parts):
    """The slices' arrays one behind the other, the slice-relative text rows rebased by the running counts: what one
    writer collects for the whole stream.  parts: (rstart, rend, sent, text_tok_end, text_sent_end[, ...]) per slice."""
    rs, re, se, tt, ts = [], [], [], [], []
    n_tok = n_sent = 0
    for p in parts:
        rs.append(np.asarray(p[0], np.int64)); re.append(np.asarray(p[1], np.int64)); se.append(np.asarray(p[2], np.int64))
        tt.append(np.asarray(p[3], np.int64) + n_tok); ts.append(np.asarray(p[4], np.int64) + n_sent)
        n_tok += len(p[0]); n_sent += len(p[2])

    def cat(x):
        return np.concatenate(x) if x else np.zeros(0, np.int64)
    return cat(rs), cat(re), cat(se), cat(tt), cat(ts)


def pack_blocked64_ref(start, end, span=SPAN):
    """(words uint32[n], heads HEAD64[ceil(n / 64)]) by dtk_off_block64's definition; ValueError if a segment of a block
    spans more than `span` (such a slice gets the plain arrays)."""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    n = len(start)
    words = np.zeros(n, np.uint32)
    heads = np.zeros((n + 63) // 64, HEAD64)
    for j in range(len(heads)):
        s, e = start[64 * j:64 * j + 64], end[64 * j:64 * j + 64]
        brk = next((l for l in range(1, len(s)) if s[l] < e[l - 1]), 64)
        base0 = min(int(s[:brk].min()), int(e[:brk].min()))
        base1 = min(int(s[brk:].min()), int(e[brk:].min())) if brk < len(s) else 0
        for l in range(len(s)):
            base = base0 if l < brk else base1
            a, b = int(s[l]) - base, int(e[l]) - base
            if not (0 <= a <= span and 0 <= b <= span):
                raise ValueError("block %d: lane %d lies %d / %d behind its base" % (j, l, a, b))
            words[64 * j + l] = a | b << 16
        heads[j] = (base0, base1, brk, 0)
    return words, heads


def unpack_blocked64_ref(words, heads):
    words = np.asarray(words, np.uint32)
    heads = np.asarray(heads).view(HEAD64).reshape(-1)
    i = np.arange(len(words), dtype=np.int64)
    h = heads[i >> 6]
    base = np.where((i & 63) < h["brk"], h["base0"], h["base1"]).astype(np.int64)
    return base + (words & np.uint32(0xFFFF)).astype(np.int64), base + (words >> np.uint32(16)).astype(np.int64)
