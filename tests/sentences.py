"""The sentence table (DTK_R_SENTENCES, dtk_sentence_view), in plain Python / numpy (test infrastructure).

Written from the definition in include/datok_gpu.h, not from the kernels: it is the CPU-side definition that the
kernels of dtk_sentences.hip and the host paths are compared against.

    Scan one document's calls in order.  A sentence is a maximal non-empty run of Token calls with no SentenceEnd or
    TextEnd between them; an open run is closed by a SentenceEnd, a TextEnd or the end of the calls; a boundary with
    no token since the previous one makes no row.  Row i holds the document's tokens [sen_tok_end[i - 1],
    sen_tok_end[i]), 0 at the first row.
"""
import bisect

import numpy as np

EVB_END, EVB_SEPS, EVB_TEOT, EVB_SEOT = 0, 2, 3, 4                          # datok_gpu.h DTK_EVB_*
EV_S_EOT, EV_E_EOT, EV_TOK_END, EV_S_EPS, EV_S_EPS2, EV_S_EOF, EV_E_EOF = 1, 2, 4, 8, 16, 32, 64   # test_host_logic.py


# ---- part 1: from the calls
def from_calls(calls):
    """(first token of every row, number of tokens) of one document.  calls: rows whose first field is the kind --
    0 (or "T") Token, anything else a SentenceEnd / TextEnd -- as oracle.Model.events() or evlist.oracle_calls() give
    them, or the (kind, a, b, c) rows of dtk_result_view.calls."""
    firsts, k, open_run = [], 0, False
    for c in calls:
        if c[0] in (0, "T"):
            if not open_run:
                firsts.append(k)
            open_run = True
            k += 1
        else:
            open_run = False
    return firsts, k


def rows_of(firsts, n_tok, tok_bstart, tok_bend, tok_rstart=None, tok_rend=None, text_tok_end=()):
    """One document's rows from its rows' first tokens and its token rows: dict of sen_tok_end, sen_bstart, sen_bend,
    sen_rstart, sen_rend (None without rune offsets) and text_sen_end.  A span whose token row does not exist is 0
    (documents with a status bit only)."""
    ends = list(firsts[1:]) + [n_tok] if firsts else []
    n = len(tok_bend)

    def first_of(a, dt):
        return np.array([a[f] if f < n else 0 for f in firsts], dtype=dt)

    def last_of(a, dt):
        return np.array([a[e - 1] if 1 <= e <= n else 0 for e in ends], dtype=dt)
    return dict(sen_tok_end=np.array(ends, dtype=np.uint32),
                sen_bstart=first_of(tok_bstart, np.uint32), sen_bend=last_of(tok_bend, np.uint32),
                sen_rstart=None if tok_rstart is None else first_of(tok_rstart, np.int32),
                sen_rend=None if tok_rend is None else last_of(tok_rend, np.int32),
                text_sen_end=np.array([bisect.bisect_left(firsts, int(t)) for t in text_tok_end], dtype=np.uint32))


def machine(flags_per_cursor):
    """The one-bit machine over one document's cursors 0..len: flags_per_cursor[p] holds EV_S_EOT / EV_E_EOT /
    EV_TOK_END / EV_S_EPS (EV_S_EPS2 counts as a SentenceEnd too; the tail's EV_S_EOF / EV_E_EOF open nothing).
    Returns the cursors of the sentence-first END bits."""
    f, out = True, []
    for p in np.flatnonzero(np.asarray(flags_per_cursor)).tolist():
        e = int(flags_per_cursor[p])
        if e & (EV_S_EOT | EV_E_EOT):
            f = True
        if e & EV_TOK_END:
            if f:
                out.append(p)
            f = False
        if e & (EV_S_EPS | EV_S_EPS2):
            f = True
    return out


# ---- part 2: from a delivered host result
def from_bitmaps(ev_bits, doc_off, tok_off, tok_bend, tok_bstart, tok_rstart=None, tok_rend=None, text_off=None,
                 text_tok_end=None, exact=None):
    """The whole table of a batch from the delivered arrays of one run: dict of n_sen, sen_off (uint64[n_docs + 1])
    and the arrays of rows_of(), concatenated over the documents.  f = 1 at a document's bit 0; per cursor in
    ascending order SEOT or TEOT: f = 1; END: first iff f, then f = 0; SEPS: f = 1.  A row's first token is the first
    k of the document with tok_bend[k] >= cursor.  exact: {document: calls} of the documents the exact pass walked
    (BatchResult.exact): their rows come from the calls."""
    doc_off = np.asarray(doc_off).astype(np.int64)
    n_docs = len(doc_off) - 1
    bit0 = doc_off + np.arange(n_docs + 1)
    n_bits = int(bit0[-1])

    def bits(kind):     # (bits at or behind n_bits belong to no document)
        return np.unpackbits(np.ascontiguousarray(ev_bits[kind]).view(np.uint8), bitorder="little")[:n_bits]
    end, seps, reset = bits(EVB_END), bits(EVB_SEPS), bits(EVB_TEOT) | bits(EVB_SEOT)
    flags = reset * np.uint8(EV_E_EOT) | end * np.uint8(EV_TOK_END) | seps * np.uint8(EV_S_EPS)
    parts, sen_off = [], [0]
    for d in range(n_docs):
        a, b = int(tok_off[d]), int(tok_off[d + 1])
        be = tok_bend[a:b].tolist()
        if exact and d in exact:
            firsts, n_tok = from_calls(exact[d])
            assert n_tok == b - a
        else:
            cursors = machine(flags[int(bit0[d]):int(bit0[d + 1])])
            firsts = [bisect.bisect_left(be, p) for p in cursors]
        ttok = () if text_off is None else text_tok_end[int(text_off[d]):int(text_off[d + 1])]
        parts.append(rows_of(firsts, b - a, tok_bstart[a:b], tok_bend[a:b], None if tok_rstart is None else tok_rstart[a:b],
                             None if tok_rend is None else tok_rend[a:b], ttok))
        sen_off.append(sen_off[-1] + len(firsts))
    out = dict(n_sen=sen_off[-1], sen_off=np.array(sen_off, dtype=np.uint64))
    for name, dt in (("sen_tok_end", np.uint32), ("sen_bstart", np.uint32), ("sen_bend", np.uint32), ("sen_rstart", np.int32),
                     ("sen_rend", np.int32), ("text_sen_end", np.uint32)):
        cols = [p[name] for p in parts]
        out[name] = None if any(c is None for c in cols) else (np.concatenate(cols).astype(dt) if cols else np.zeros(0, dt))
    return out
