"""The corpus of tests/test_symbolize_lanes.py (tests/symlanes.py) checked on the CPU, before any GPU is asked: it
holds what it claims, and the reference agrees with the second, independent decoder on all of it, the way
tests/test_symref.py checks the first corpus."""
import numpy as np

import symlanes
import symref

from datok_amd.host import _decode_runes


def _batches():
    for c in symlanes.corpora():
        yield c
    for n in symlanes.SMALL:
        yield ("small/%d" % n,) + symlanes.small(n)


def test_the_lane_corpus_holds_what_it_claims():
    seqs = symref.sequences()
    text, off = symlanes.lane_edges()
    assert len(text) == (len(seqs) * 64 + 1) * symlanes.ROW and int(off[-1]) == len(text)
    assert np.all(off[1:-1] % symlanes.ROW == symlanes.DOC_SHIFT)          # no document boundary on a KiB boundary
    raw, residues = text.tobytes(), set()
    for i, s in enumerate(seqs):
        for r in range(64):
            row = (i * 64 + r) * symlanes.ROW
            for b in symlanes.EDGE_BASES:
                at = row + b + r
                assert raw[at - 1:at + len(s) + 1] == b" " + s + b" ", (i, r, b)
                residues.add((b, at % 64))
            if r + len(s) > 32 > r:                                        # across the KiB boundary: one document
                assert symref.doc_of(off, row + symlanes.ROW - 1) == symref.doc_of(off, row + symlanes.ROW)
    assert len(residues) == 4 * 64 and {(symlanes.ROW, r) for r in range(64)} <= residues   # counted from the KiB boundary too
    assert sum(c >= 0x80 for c in raw) == 4 * 64 * sum(c >= 0x80 for s in seqs for c in s)

    text, off = symlanes.lane_cuts()
    lens = np.diff(off.astype(np.int64))
    rows = len(text) // symlanes.CUT_ROW
    assert symlanes.CUTS == (0, 1, 2, 71)        # no boundary, a plain one, runs of 1 and of 70 empty documents
    assert rows == len(symlanes.CUTS) * len(seqs) * len(symlanes.CUT_AT) * 17 and lens.max() <= symlanes.CUT_ROW
    per = rows // len(symlanes.CUTS)
    assert int((lens == 0).sum()) == (1 + 70) * per
    cut_in_lane = {int(o) % symlanes.CUT_ROW for o in off[1:-1]}
    assert cut_in_lane == {0} | set(range(symlanes.LANE, 2 * symlanes.LANE + 1))
    # the offsets of a block without, with a plain boundary and with single empty documents fit the kernels' 256 in
    # LDS -- and blocks of the third kind hold empty documents at every offset 0..16 of a lane --, those with runs
    # of 70 do not
    edges = np.arange(0, len(text) + 1, symref.BLOCK)
    n_in = np.diff(np.searchsorted(off, edges))
    per_blocks = per * symlanes.CUT_ROW // symref.BLOCK
    assert n_in[:3 * per_blocks - 1].max() + 3 <= 256 and n_in[3 * per_blocks + 1:].min() > 1000
    empty_at = off[:-1][lens == 0].astype(np.int64)
    single = empty_at[(empty_at >= 2 * per * symlanes.CUT_ROW) & (empty_at < 3 * per * symlanes.CUT_ROW)]
    assert len(single) == per and len(np.unique(single)) == per
    assert {int(o) % symlanes.CUT_ROW for o in single} == set(range(symlanes.LANE, 2 * symlanes.LANE + 1))

    text, off = symlanes.block_cuts()
    assert {int(o) % symref.BLOCK for o in off[1:-1]} == {symref.BLOCK - 3, symref.BLOCK - 2, symref.BLOCK - 1, 0, 1}
    starts = symref.decode_stream(text, off)[1] > 0
    edges = np.arange(symref.BLOCK, len(text), symref.BLOCK)
    assert not starts[edges].all() and starts[edges].any()    # a block's first byte covered from the block in front, and not

    text, off = symlanes.uneven_loops()
    leads = (text >= 0xC0).reshape(-1, symlanes.LANE).sum(axis=1)
    assert len(off) == 2 and len(text) % symref.BLOCK == 0 and leads.max() == 16
    for wave, (size, most) in enumerate(((2, 8), (2, 8), (3, 5), (3, 5), (1, 16), (1, 16), (1, 16), (1, 16))):
        per_lane = (text[wave * 1024:(wave + 1) * 1024] >= 0x80).reshape(64, symlanes.LANE).sum(axis=1) // size
        rising = [l % (most + 1) for l in range(64)]
        assert per_lane.tolist() == (rising if wave % 2 == 0 else rising[::-1]), wave
    starts = symref.decode_stream(text, off)[1] > 0
    covered = {(int(p) % symref.BLOCK == 0, int(p) % 1024 == 0, n)
               for p in range(0, len(text), symlanes.LANE) for n in (1, 2, 3)
               if not starts[p:p + n].any() and (n == 3 or starts[p + n])}
    for n in (1, 2, 3):      # the first n bytes covered: of a lane inside a wave, of a wave's first, of a block's first
        assert {(False, False, n), (False, True, n), (True, True, n)} <= covered, n
    assert symlanes.SMALL[:80] == tuple(range(1, 81)) and {1007, 1023, 1025, 1041} <= set(symlanes.SMALL)


def test_reference_and_the_host_decoder_agree_on_the_lane_corpus():
    """decode_stream (Go's DecodeRune through the oracle, run by run) against datok_amd.host._decode_runes (pure
    Python, document by document): the same runes at the same boundaries, on every batch of the lane tests."""
    checked = 0
    for name, text, off in _batches():
        rune, width = symref.decode_stream(text, off)
        low = text < 0x80
        assert np.array_equal(rune[low], text[low]) and np.all(width[low] == 1), name
        raw, o = text.tobytes(), off.astype(np.int64)
        hi = np.flatnonzero(~low)
        pos = 0
        while pos < len(hi):            # every stretch of bytes >= 0x80 with the byte behind it, inside its document
            i = int(hi[pos])
            dend = int(o[symref.doc_of(o, i) + 1])
            e = i
            while e < dend and raw[e] >= 0x80:
                e += 1
            piece = raw[i:min(e + 1, dend)]
            starts = [k for k in range(len(piece)) if width[i + k]]
            assert starts[0] == 0 and _decode_runes(piece) == [int(rune[i + k]) for k in starts], (name, i, piece[:16].hex())
            assert sum(int(width[i + k]) for k in starts) == len(piece), (name, i)
            checked += len(starts)
            pos = int(np.searchsorted(hi, e))
        lens = np.diff(o)
        for d in range(0, len(o) - 1, 7):   # and whole documents, every seventh
            a, b = int(o[d]), int(o[d + 1])
            if 0 < b - a <= 16384:
                assert _decode_runes(raw[a:b]) == rune[a:b][width[a:b] > 0].tolist(), (name, d)
        assert int(lens.sum()) == len(text)
    assert checked > 40000
