"""The symboliser's reference and corpus (tests/symref.py) checked on the CPU, before any GPU is asked: the reference
agrees with a second, independent decoder on every corpus, passes Go's decoder vectors, the corpus holds what it
claims, and the comparison the GPU tests rely on does fail -- and says where -- when one entry or one bit is wrong."""
import gzip
import os

import numpy as np
import pytest

import craft
import symref
from conftest import MODELS
from test_oracle_golden import GO_UTF8_VECTORS

from datok_amd.host import _decode_runes


def _crafted():
    from oracle import oracle as O
    blob, extra = craft.big_sigma("matok")
    return O.Model(raw=gzip.decompress(blob)), [extra[k].encode() for k in (0, 39, 40, 299)]


def _corpora(extra=()):
    """(name, text, doc_off) of every batch the GPU tests run."""
    text, what = symref.rows(extra)
    for lay in "abc":
        yield "rows/" + lay, text, symref.layout(len(what), lay)
    for first in (8192, symref.ROW + 8192 - 1):    # the 8192 - j placement of row 0 (j = 0) and of row 1 (j = 1) as byte 0
        sub = text[first:]
        yield "rows/c from %d" % first, sub, symref.layout(0, "c", len(sub))
    for n in symref.TAILS:
        yield ("tail/%d" % n,) + symref.tail(n)
    yield ("dense",) + symref.dense()
    yield ("empty runs",) + symref.empty_runs()


def test_the_corpus_holds_what_it_claims():
    seqs = symref.sequences()
    assert len(seqs) >= 40 and len(set(seqs)) == len(seqs)
    text, what = symref.rows()
    assert len(what) >= 148 and len(what) == sum(len(s) + 1 for s in seqs) and len(text) == len(what) * symref.ROW
    assert symref.ROW % symref.BLOCK == 0
    placed = 0
    for r, (s, j) in enumerate(what):
        row = text[r * symref.ROW:(r + 1) * symref.ROW].tobytes()
        for B in symref.EDGES:
            assert row[B - j:B - j + len(s)] == s and row[B - j - 1] == 32 and row[B - j + len(s)] == 32, (r, B)
            placed += 1
        high = sum(c >= 0x80 for c in row)
        assert high == 5 * sum(c >= 0x80 for c in s)            # nothing but the placements is not ASCII
    assert placed == 5 * len(what)
    assert len(symref.layout(len(what), "a")) - 1 == len(what)
    assert len(symref.layout(len(what), "b")) - 1 == 6 * len(what)
    c = symref.layout(len(what), "c")
    assert np.all(np.diff(c) == 8) and symref.BLOCK // 8 > symref.BLOCK // 16    # more documents per block than SYM_DOFF
    for n in symref.TAILS:
        t, off = symref.tail(n)
        assert len(t) == n and int(off[-1]) == n and (n < 3 or (t[0] == 0x80 and bytes(t[-2:]) == b"\xe2\x82"))
    assert {n % 4 for n in symref.TAILS} == {0, 1, 2, 3}
    t, off = symref.dense()
    lens = np.diff(off.astype(np.int64))
    for d in range(1, len(lens), 3):                            # the payload documents: nothing below 0x80
        assert lens[d] >= 1024 and t[int(off[d]):int(off[d + 1])].min() >= 0x80
        assert int(off[d]) % 1024 == (0 if d % 6 == 1 else 1)    # on a quarter edge / one byte behind it
    t, off = symref.empty_runs()
    lens = np.diff(off.astype(np.int64))
    runs = {}
    for at in np.unique(off[:-1][lens == 0]).tolist():
        runs[at] = int(np.sum((off[:-1] == at) & (lens == 0)))
    assert set(runs.values()) == {70, 4100} and {0, 4096, 4097, 8192, 8193, len(t)} <= set(runs)


@pytest.mark.parametrize("extra", [False, True], ids=["shipped", "crafted"])
def test_reference_and_the_host_decoder_agree_on_every_corpus(extra):
    """decode_stream (Go's DecodeRune through the oracle, run by run) against datok_amd.host._decode_runes (pure
    Python, document by document): the same runes at the same boundaries."""
    checked = 0
    for name, text, off in _corpora(_crafted()[1] if extra else ()):
        rune, width = symref.decode_stream(text, off)
        low = text < 0x80
        assert np.array_equal(rune[low], text[low]) and np.all(width[low] == 1), name
        raw, o = text.tobytes(), off.astype(np.int64)
        # every stretch of bytes >= 0x80 with the byte behind it, document by document: values, and boundaries --
        # decoding from any rune start gives the rest of the same runes
        hi = np.flatnonzero(~low)
        pos = 0
        while pos < len(hi):
            i = int(hi[pos])
            d = symref.doc_of(o, i)
            dend = int(o[d + 1])
            e = i
            while e < dend and raw[e] >= 0x80:
                e += 1
            piece = raw[i:min(e + 1, dend)]
            starts = [k for k in range(len(piece)) if width[i + k]]
            assert starts[0] == 0 and _decode_runes(piece) == [int(rune[i + k]) for k in starts], (name, i, piece[:16].hex())
            assert sum(int(width[i + k]) for k in starts) == len(piece), (name, i)
            for n, k in enumerate(starts if len(piece) <= 64 else starts[::97]):
                tail_runes = [int(rune[i + q]) for q in starts if q >= k]
                assert _decode_runes(piece[k:]) == tail_runes, (name, i, k)
            checked += len(starts)
            pos = int(np.searchsorted(hi, e))
        # and whole documents, every seventh
        for d in range(0, len(o) - 1, 7):
            a, b = int(o[d]), int(o[d + 1])
            if b - a <= 16384:
                assert _decode_runes(raw[a:b]) == rune[a:b][width[a:b] > 0].tolist(), (name, d)
    assert checked > 10000


def test_go_decoder_vectors_through_the_reference(oracle_models):
    om = oracle_models("tokenizer_de.matok")
    for b, (r, w) in GO_UTF8_VECTORS:
        text, off = np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.uint64)
        rune, width = symref.decode_stream(text, off)
        assert (int(rune[0]), int(width[0])) == (r, w), b
        entries, starts, saw = symref.reference_stream(om, text, off)
        assert int(entries[0]) >> symref.W_SHIFT & 7 == w and bool(starts[0]) and saw == (r == 0xFFFD), b
        assert int(starts.sum()) == len(b) - w + 1               # what follows an invalid byte starts runes of its own
    # symbol and class as matrix.go:421-435 picks them
    e = symref.reference_stream(om, np.frombuffer("a\x04ä“日".encode(), dtype=np.uint8), np.array([0, 10], dtype=np.uint64))[0]
    asc = om.sigma_ascii()
    assert [int(x) >> symref.CLS_SHIFT for x in e[[0, 1, 2, 4, 7]]] == [0, 1, 0, 2, 3]
    assert [int(x) & symref.SYM_MASK for x in e[[0, 1, 2, 7]]] == [asc[97], asc[4], asc[0xE4], om.info["identity"]] and int(e[4]) & symref.SYM_MASK > 3
    # a document boundary cuts a rune into invalid pieces
    text = np.frombuffer("€".encode(), dtype=np.uint8)
    assert symref.reference_stream(om, text, np.array([0, 3], dtype=np.uint64))[1].tolist() == [True, False, False]
    assert symref.reference_stream(om, text, np.array([0, 1, 3], dtype=np.uint64))[1].tolist() == [True, True, True]
    assert symref.reference_stream(om, text, np.array([0, 2, 2, 3], dtype=np.uint64))[2] is True


def test_the_comparison_fails_and_says_where(oracle_models):
    """One wrong entry, one wrong width, one wrong bitmap bit, a bit behind the end, the wrong flag: each makes
    assert_stream_equal fail, naming the byte and its document."""
    om = oracle_models("tokenizer_de.matok")
    text, what = symref.rows()
    text, n_rows = text[:4 * symref.ROW + 13], 4
    off = np.append(symref.layout(n_rows, "b"), len(text)).astype(np.uint64)
    ref = symref.reference_stream(om, text, off)
    good = (ref[0].copy(), symref.pack_bits(ref[1]), ref[2])
    symref.assert_stream_equal(good, ref, text, off, "identical")
    assert len(good[1]) == (len(text) + 31) // 32
    pos = symref.ROW + 4096 + 5                       # byte 5 of document 10 (row 1, the piece that begins at 4096)
    assert symref.doc_of(off, pos) == 10 and int(off[10]) == pos - 5 and ref[1][pos]

    def failing(entries=None, words=None, flag=None):
        got = (good[0] if entries is None else entries, good[1] if words is None else words, good[2] if flag is None else flag)
        with pytest.raises(AssertionError) as e:
            symref.assert_stream_equal(got, ref, text, off, "mutated")
        return str(e.value)
    e = good[0].copy(); e[pos] ^= 1                   # another symbol
    msg = failing(entries=e)
    assert "entry" in msg and "byte 5 of document 10" in msg and "byte %d of the batch" % pos in msg
    e = good[0].copy(); e[pos] ^= 1 << symref.CLS_SHIFT
    assert "byte 5 of document 10" in failing(entries=e)
    e = good[0].copy(); e[pos] ^= 1 << symref.W_SHIFT
    msg = failing(entries=e)
    assert "width" in msg and "byte 5 of document 10" in msg
    cont = int(np.flatnonzero(~ref[1])[0])             # a continuation byte: only its width counts ...
    e = good[0].copy(); e[cont] ^= 0x7FF
    symref.assert_stream_equal((e, good[1], good[2]), ref, text, off, "symbol bits of a continuation byte")
    e[cont] |= 1 << symref.W_SHIFT                       # ... but that does
    assert "width differs at byte %d of document %d" % (cont - int(off[symref.doc_of(off, cont)]), symref.doc_of(off, cont)) in failing(entries=e)
    w = good[1].copy(); w[pos >> 5] ^= np.uint32(1 << (pos & 31))
    msg = failing(words=w)
    assert "rune-start bit" in msg and "byte 5 of document 10" in msg
    w = good[1].copy(); w[-1] |= np.uint32(1 << 31)    # (the batch ends 13 bytes into its last word)
    assert "behind the batch" in failing(words=w)
    assert "saw_invalid" in failing(flag=not good[2])
