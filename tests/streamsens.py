"""The reference of a stream's sentence rows (test infrastructure): tests/test_stream_sentences_host.py,
tests/test_stream_sentences.py.

Written from the definition in include/datok_gpu.h (dtk_stream_set_sentences), not from the kernels: scan the stream's
calls in order; a sentence is a maximal non-empty run of Token calls with no SentenceEnd or TextEnd between them; a row
is delivered by the slice whose calls close it (on the last slice also by the end of the calls), and the row that is
open at a cut crosses it as (open, bstart, bend, rstart, rend).  sentences_slice_ref walks one slice's calls -- the
tokens merged with the event list by cursor, exactly as streamoffs.offsets_slice_ref merges them, whose rune offsets it
takes --; join_sentences puts the slices' rows one behind the other; stream_table is the table of the whole stream from
the oracle's calls (sentences.from_calls + sentences.rows_of).
"""
import numpy as np

import sentences as sn
from datok_amd.host import EVL_SEOT, EVL_SEPS, EVL_TEOT
from streamoffs import offsets_slice_ref

SEN_CARRY0 = (False, 0, 0, 0, 0)
SIX = ("sen_tok_end", "sen_bstart", "sen_bend", "sen_rstart", "sen_rend", "text_sen_end")


def sentences_slice_ref(is_matrix, sl, nl, carry_in, sen_carry_in):
    """(sen_tok_end, sen_bstart, sen_bend, sen_rstart, sen_rend, text_sen_end, sen_carry_out) of the slice `sl` (a
    SliceView): the rows its calls close.  carry_in: the writer's state in front of the slice (offsets_slice_ref's);
    sen_carry_in: the open row, (open, bstart, bend, rstart, rend)."""
    rstart, rend = offsets_slice_ref(is_matrix, sl, nl, carry_in)[:2]
    n = len(sl.text)
    base = int(sl.base)
    is_open, bs, be, rs, re = sen_carry_in
    rows, tse = [], []

    def close():
        nonlocal is_open
        if is_open:
            rows.append((k, bs, be, rs, re))
        is_open = False

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
            close()
        if e & EVL_TEOT:
            close()
            tse.append(len(rows))
        if pt == p:
            if not is_open:
                is_open, bs, rs = True, base + int(sl.tok_bstart[k]), int(rstart[k])
            be, re = base + min(pt, n), int(rend[k])
            k += 1
        if e & EVL_SEPS:
            close()
    if sl.last:
        if int(sl.tail) & 1:
            close()
        if int(sl.tail) & 2:
            close()
            tse.append(len(rows))
        close()                                    # the end of the calls
    r = np.array(rows, dtype=object).reshape(len(rows), 5)
    carry_out = (True, bs, be, rs, re) if is_open else SEN_CARRY0
    return (r[:, 0].astype(np.uint32), r[:, 1].astype(np.uint64), r[:, 2].astype(np.uint64), r[:, 3].astype(np.int64),
            r[:, 4].astype(np.int64), np.array(tse, np.uint32), carry_out)


def join_sentences(parts):
    """The slices' rows one behind the other: sen_tok_end rebased by the running token count, text_sen_end by the running
    row count.  parts: (n_tok of the slice, sen_tok_end, sen_bstart, sen_bend, sen_rstart, sen_rend, text_sen_end) per
    slice.  Returns the six arrays as int64."""
    cols = [[] for _ in SIX]
    n_tok = n_sen = 0
    for p in parts:
        cols[0].append(np.asarray(p[1], np.int64) + n_tok)
        for c, a in zip(cols[1:5], p[2:6]):
            c.append(np.asarray(a).astype(np.int64))
        cols[5].append(np.asarray(p[6], np.int64) + n_sen)
        n_tok += int(p[0]); n_sen += len(p[1])
    return tuple(np.concatenate(c) if c else np.zeros(0, np.int64) for c in cols)


def stream_table(calls, doc, n_tok=None):
    """The whole stream's table from the oracle's calls (streamcorpus.oracle_calls) and the oracle's rune offsets and text
    rows (`doc`: oracle.Model.transduce_doc of the same stream): the six arrays as int64.  n_tok: only the calls in
    front of that many tokens' successor count (a stream the reference ends early)."""
    if n_tok is not None:
        upto, seen = len(calls), 0
        for i, c in enumerate(calls):
            if c[0] == 0:
                if seen == n_tok:
                    upto = i
                    break
                seen += 1
        calls = calls[:upto]
    firsts, nt = sn.from_calls(calls)
    toks = [c for c in calls if c[0] == 0]
    t = sn.rows_of(firsts, nt, [c[3] for c in toks], [c[4] for c in toks], np.asarray(doc.tok_rstart)[:nt],
                   np.asarray(doc.tok_rend)[:nt], [x for x in np.asarray(doc.text_tok_end).tolist() if x <= nt])
    return tuple(np.asarray(t[name]).astype(np.int64) for name in SIX)


def assert_table(got, want, what=(), only=SIX):
    for name, g, w in zip(SIX, got, want):
        if name not in only:
            continue
        assert len(g) == len(w), (what, name, len(g), len(w))
        bad = np.flatnonzero(np.asarray(g, np.int64) != np.asarray(w, np.int64))
        assert len(bad) == 0, (what, name, int(bad[0]), g[bad[:3]], w[bad[:3]])
