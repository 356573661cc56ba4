"""Corpus for the edges of a symboliser that decodes in registers (test infrastructure, CPU only): a lane owns 16
consecutive bytes, a wave 64 lanes (1 KiB), a block four waves (4 KiB); a lane looks three bytes ahead into its
neighbour (the wave's last lane into a halo word) and learns from its neighbour which of its first three bytes the
sequence in front covers (the wave's first lane decodes the bytes in front of it itself).  Built from symref's
sequences and filler; no random numbers.  Every builder returns (uint8 text, uint64 doc_off)."""
import numpy as np

import symref

LANE, WAVE_BYTES, BLOCK = 16, 1024, symref.BLOCK
ROW = WAVE_BYTES
EDGE_BASES = (256, 512, ROW - 32, ROW)   # inside a quarter (row-of-16-lanes and half-wave edges); up to and over the
                                         # KiB boundary; counted from the KiB boundary (the next row's first bytes)
DOC_SHIFT = 128                       # lane_edges: a document begins this far into every row
CUT_ROW, CUT_AT = 64, (6, 14)         # lane_cuts: 64-byte rows; the sequence 6 or 14 bytes into the row's second lane
CUTS = (0, 1, 2, 71)                  # boundaries at one offset: none, a plain one, a run of 1 and of 70 empty documents
BLOCK_CUT_SEQS = ("c3a4", "e2809c", "f09f9880")
SMALL = tuple(range(1, 81)) + tuple(n for d in range(1, 18) for n in (1024 - d, 1024 + d))


def _arr(buf):
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy()


def _put(buf, at, s):
    """s at `at`, a blank on either side."""
    buf[at - 1:at + len(s) + 1] = b" " + s + b" "


def _offsets(total, cuts):
    """cuts: {offset: boundaries there}; k boundaries at one offset are k - 1 empty documents."""
    off = [0]
    for at in sorted(cuts):
        assert 0 < at < total
        off += [at] * cuts[at]
    return np.array(off + [total], dtype=np.uint64)


def lane_edges(extra=()):
    """One KiB row per (sequence, residue 0..63): the sequence at 256 + r and 512 + r of its row -- before, across at
    every split, and behind every 8-, 16-, 32- and 64-byte edge inside a wave --, at 992 + r, where it runs up to
    and over the KiB boundary into the next row, and at 1024 + r, the residue counted from the KiB boundary (the next
    row's first 69 bytes belong to the row in front): the wave's last lane looks into its halo, the next wave's first
    lane decodes what lies in front of it; every fourth boundary is a block's.  Documents of one KiB that begin 128
    bytes into a row, so every KiB boundary lies inside a document."""
    seqs = symref.sequences(extra)
    n = len(seqs) * 64
    buf = bytearray(symref.filler((n + 1) * ROW))
    for i, s in enumerate(seqs):
        for r in range(64):
            for b in EDGE_BASES:
                _put(buf, (i * 64 + r) * ROW + b + r, s)
    return _arr(buf), _offsets(len(buf), {at: 1 for at in range(DOC_SHIFT, len(buf), ROW)})


def lane_cuts(extra=(), cuts_at_once=CUTS):
    """Document boundaries inside a lane.  64-byte rows, each beginning a document; the sequence 6 bytes into the
    row's second lane (inside it) or 14 bytes into it (across the lane edge); k boundaries (k - 1 empty documents)
    at every byte offset 0..16 of that lane in turn -- in front of the sequence, through it at every split, on the
    lane edge, behind it.  Rows of one k follow each other: the blocks of k = 0, 1 and 2 keep their document offsets
    in LDS (65, 129 and 193 a block; k = 2: equal offsets in that table), those of k = 71 search them in memory."""
    seqs = symref.sequences(extra)
    base_row = symref.filler(CUT_ROW)
    buf, cuts = bytearray(), {}
    for run in cuts_at_once:
        for s in seqs:
            for at in CUT_AT:
                for t in range(17):
                    start = len(buf)
                    buf += base_row
                    _put(buf, start + LANE + at, s)
                    if start:
                        cuts[start] = 1
                    if run:
                        cuts[start + LANE + t] = run
    return _arr(buf), _offsets(len(buf), cuts)


def block_cuts(cuts_at_once=CUTS):
    """The same across a block's first byte: a sequence j bytes in front of a 4 KiB boundary and the rest behind it,
    and k document boundaries (k - 1 empty documents) 3, 2, 1 or 0 bytes in front of that boundary or 1 byte behind
    it: the lead byte that the block's first lane looks back at lies in a document that ends in front of the block,
    at it, or goes on."""
    cases = [(run, bytes.fromhex(h), j, t) for run in cuts_at_once for h in BLOCK_CUT_SEQS
             for j in range(1, len(bytes.fromhex(h))) for t in (-3, -2, -1, 0, 1)]
    buf, cuts = bytearray(symref.filler((len(cases) + 1) * BLOCK)), {}
    for i, (run, s, j, t) in enumerate(cases):
        edge = (i + 1) * BLOCK
        _put(buf, edge - j, s)
        if run:
            cuts[edge + t] = run
    return _arr(buf), _offsets(len(buf), cuts)


def _wave(counts, unit, pad=b" "):
    """1 KiB: lane l holds counts[l] copies of `unit` and blanks."""
    out = bytearray()
    for c in counts:
        assert c * len(unit) <= LANE
        out += unit * c + pad * (LANE - c * len(unit))
    return bytes(out)


def uneven_loops():
    """Waves whose lanes hold 0, 1, 2, ... up to as many as fit of: c3a4 (8), e2809c (5), a bare c3 (16 lead bytes:
    the most a lane can hold), a stray 80 (16), in rising and in falling order across the lanes; then lanes whose
    last sequence covers the first one, two or three bytes of the next lane, in the middle of a wave, in its last lane
    (the next wave's first lane) and in a block's last lane (the next block's first lane).  One document, and the
    same text again in documents of 48 bytes (lanes that begin and end documents between their lead bytes)."""
    waves = []
    for unit, most in ((b"\xc3\xa4", 8), (b"\xe2\x80\x9c", 5), (b"\xc3", 16), (b"\x80", 16)):
        rising = [l % (most + 1) for l in range(64)]
        waves += [_wave(rising, unit), _wave(rising[::-1], unit)]
    buf = bytearray(b"".join(waves))
    buf += symref.filler(-len(buf) % BLOCK)
    spills = [(bytes.fromhex(h), back) for h, backs in (("c3a4", (1,)), ("e2809c", (1, 2)), ("f09f9880", (1, 2, 3)), ("e28241", (1, 2)))
              for back in backs]       # (e28241: a lead byte whose sequence is cut short by a letter covers nothing)
    for s, back in spills:             # two blocks each: a lane edge inside a wave, a wave's edge, a block's edge
        base = len(buf)
        buf += symref.filler(2 * BLOCK)
        for edge in (base + 4 * LANE, base + WAVE_BYTES, base + BLOCK):
            _put(buf, edge - back, s)
    text = _arr(buf)
    return text, np.array([0, len(text)], dtype=np.uint64)


def uneven_loops_cut():
    text, _ = uneven_loops()
    return text, _offsets(len(text), {at: 1 for at in range(48, len(text), 48)})


def small(n):
    """symref.tail(n): 0x80 first, a truncated e2 82 last."""
    return symref.tail(n)


def corpora(extra=()):
    """(name, text, doc_off) of every batch of tests/test_symbolize_lanes.py but the small ones."""
    yield ("lane edges",) + lane_edges(extra)
    yield ("lane cuts",) + lane_cuts(extra)
    yield ("block cuts",) + block_cuts()
    yield ("uneven loops",) + uneven_loops()
    yield ("uneven loops, cut",) + uneven_loops_cut()
