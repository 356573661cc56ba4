"""The definition of an encoding in plain Python (test infrastructure): tests/test_encode_host.py, tests/test_encode.py.
It restates include/datok_gpu.h (dtk_batch_set_encode).

A unit is a token range [t0, t1) of the batch with its document's first token tok0; its pieces are
piece_id[piece_off[t0]:piece_off[t1]], n of them.  With body = max_len - n_special and step = body - stride:
  windows   1 if n <= body or first_window, else 1 + ceil((n - body) / step); window k holds the unit's pieces
            [k * step, min(k * step + body, n))
  a row     cls_id if >= 0, the window's pieces, sep_id if >= 0, pad_id up to max_len
  row_len   the positions in front of the padding; row_piece0 the batch-wide index of the row's first body piece
  word_id   per body position the document-relative index of the piece's token, -1 elsewhere
"""
import numpy as np


class Spec:
    def __init__(self, max_len, cls_id=-1, sep_id=-1, pad_id=0, stride=0, first_window=False, word_ids=False):
        self.max_len, self.cls_id, self.sep_id, self.pad_id = max_len, cls_id, sep_id, pad_id
        self.stride, self.first_window, self.word_ids = stride, first_window, word_ids
        self.n_special = (cls_id >= 0) + (sep_id >= 0)
        self.body = max_len - self.n_special
        self.step = self.body - stride

    def kw(self):
        """The keyword arguments of Batch.set_encode / encode_rows that state this spec."""
        return dict(max_len=self.max_len, cls_id=self.cls_id, sep_id=self.sep_id, pad_id=self.pad_id, stride=self.stride,
                    first_window=self.first_window, word_ids=self.word_ids)


def windows(spec, n):
    """[(first, end)] of a unit of n pieces, relative to the unit."""
    if n <= spec.body or spec.first_window:
        return [(0, min(n, spec.body))]
    w = 1 + -(-(n - spec.body) // spec.step)
    return [(k * spec.step, min(k * spec.step + spec.body, n)) for k in range(w)]


def tokens_of_pieces(piece_off, t0, t1):
    """{piece: its token} for the tokens [t0, t1): token t owns the pieces [piece_off[t], piece_off[t + 1]), a token
    without a piece owns none."""
    return {q: t for t in range(t0, t1) for q in range(int(piece_off[t]), int(piece_off[t + 1]))}


def expected(spec, units, piece_off, piece_id):
    """units: [(t0, t1, tok0)].  Returns a dict of the outputs as numpy arrays and counts."""
    off, ids, lens, p0s, words, n_cut = [0], [], [], [], [], 0
    for t0, t1, tok0 in units:
        a, z = int(piece_off[t0]), int(piece_off[t1])
        n = z - a
        n_cut += n > spec.body
        owner = tokens_of_pieces(piece_off, t0, t1) if spec.word_ids else {}
        for first, end in windows(spec, n):
            body = [int(x) for x in piece_id[a + first:a + end]]
            row = ([spec.cls_id] if spec.cls_id >= 0 else []) + body + ([spec.sep_id] if spec.sep_id >= 0 else [])
            lens.append(len(row))
            ids.append(row + [spec.pad_id] * (spec.max_len - len(row)))
            p0s.append(a + first)
            if spec.word_ids:
                w = [owner[q] - tok0 for q in range(a + first, a + end)]
                w = ([-1] if spec.cls_id >= 0 else []) + w
                words.append(w + [-1] * (spec.max_len - len(w)))
        off.append(len(ids))
    return dict(unit_row_off=np.array(off, np.uint64), input_ids=np.array(ids, np.int32).reshape(-1, spec.max_len),
                row_len=np.array(lens, np.uint32), row_piece0=np.array(p0s, np.uint64),
                word_id=np.array(words, np.int32).reshape(-1, spec.max_len) if spec.word_ids else None,
                n_units=len(units), n_rows=len(ids), n_cut=int(n_cut))


def units_of_documents(tok_off):
    """DOCUMENT: one unit per document, also one without a token."""
    return [(int(tok_off[d]), int(tok_off[d + 1]), int(tok_off[d])) for d in range(len(tok_off) - 1)]


def units_of_sentences(tok_off, sen_off, sen_tok_end):
    """SENTENCE: one unit per row of the sentence table; row i of document d holds the document's tokens
    [sen_tok_end[i - 1], sen_tok_end[i]), from 0 at the document's first row."""
    units = []
    for d in range(len(tok_off) - 1):
        t = int(tok_off[d])
        for i in range(int(sen_off[d]), int(sen_off[d + 1])):
            first = 0 if i == int(sen_off[d]) else int(sen_tok_end[i - 1])
            units.append((t + first, t + int(sen_tok_end[i]), t))
    return units


def assert_equal(got, exp, what=""):
    """An Encoded (datok_amd) against expected(): every array and every count, exactly."""
    assert (got.n_units, got.n_rows, got.n_cut) == (exp["n_units"], exp["n_rows"], exp["n_cut"]), \
        (what, got.n_units, got.n_rows, got.n_cut, exp["n_units"], exp["n_rows"], exp["n_cut"])
    assert got.input_ids.dtype == np.int32 and got.row_len.dtype == np.uint32
    assert got.unit_row_off.dtype == np.uint64 and got.row_piece0.dtype == np.uint64
    for name in ("unit_row_off", "row_len", "row_piece0", "input_ids"):
        g, e = getattr(got, name), exp[name]
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        bad = np.argwhere(g != e)
        assert not len(bad), (what, name, bad[:4].tolist(), g[tuple(bad[0])], e[tuple(bad[0])])
    if exp["word_id"] is None:
        assert got.word_id is None, what
    else:
        assert got.word_id is not None and got.word_id.dtype == np.int32 and got.word_id.shape == exp["word_id"].shape, what
        bad = np.argwhere(got.word_id != exp["word_id"])
        assert not len(bad), (what, "word_id", bad[:4].tolist(), got.word_id[tuple(bad[0])], exp["word_id"][tuple(bad[0])])
    mask = got.attention_mask()
    assert mask.shape == got.input_ids.shape and np.array_equal(mask.sum(axis=1), got.row_len.astype(np.int64)), what
