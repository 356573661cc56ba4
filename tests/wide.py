"""Tokenizers of 32 767 states and more, made by the tests (test infrastructure; nothing of this size is committed).

The fused table cells of the device have 15-bit state ids in their 32-bit form and 30-bit ids in their 64-bit form
(datok_amd/csrc/dtk_model.cpp, pick_encoding); no shipped model needs the second.  Two recipes give models that do:

widen_matok   scatters the n states of a real `.matok` over the ids 1..N (state 1 stays 1; a seeded random injection,
              targets remapped, the other rows empty).  The automaton is the same one, so the oracle's output for the
              ORIGINAL file -- which the reference's goldens pin -- is the expected value.
trie_automaton  craft._automaton with its one "inside a word" state replaced by a binary trie over a / b of depth 15:
              65 541 states, every one reachable, high ids visited by any text with words of a few letters, and the walk
              re-synchronises at every token like the base automaton.  The expected values are those of craft.matok() /
              craft.datok().
"""
import gzip
import struct

import numpy as np

import craft

FIRST = np.uint32(1 << 31)
TRIE_DEPTH = 15
TRIE_STATES = 65541          # of trie_automaton(); two more with triple=True (the base automaton has two more)


def parse_matok(gz: bytes):
    """(header fields, sigma bytes, symbol-major array) of a `.matok` image (matrix.go:126-210)."""
    raw = gzip.decompress(gz)
    assert raw[:5] == b"MATOK"
    ver, eps, unk, ident, n, s = struct.unpack_from("<HHHHIH", raw, 5)
    off = 19
    for _ in range(s):                       # the sigma: s runes of UTF-8, NUL = no character
        b = raw[off]
        off += 1 if b < 0x80 else 2 if b < 0xE0 else 3 if b < 0xF0 else 4
    assert raw[off:off + 1] == b"M"
    arr = np.frombuffer(raw, dtype="<u4", count=(n + 1) * s, offset=off + 1)
    return (ver, eps, unk, ident, n, s), raw[19:off], arr


def widen_matok(gz: bytes, n_states: int, seed=7) -> bytes:
    """The same automaton with its states scattered over 1..n_states, as MatrixTokenizer.WriteTo lays it out."""
    (ver, eps, unk, ident, n, s), sig, arr = parse_matok(gz)
    N = int(n_states)
    assert N >= n
    rng = np.random.default_rng(seed)
    newid = np.zeros(n + 1, dtype=np.uint32)
    ids = np.sort(rng.choice(np.arange(2, N + 1), size=n - 1, replace=False)).astype(np.uint32)
    newid[1] = 1
    newid[2:] = ids[rng.permutation(n - 1)]
    out = np.zeros((N + 1) * s, dtype=np.uint32)
    for a in range(1, s):
        col = arr[(a - 1) * n + 1:(a - 1) * n + n + 1]          # array[(a-1)*stateCount + t], t = 1..n (matrix.go:463)
        tgt, flag = col & ~FIRST, col & FIRST
        v = np.where(tgt != 0, newid[np.minimum(tgt, n)] | flag, 0).astype(np.uint32)
        out[(a - 1) * N + newid[1:]] = v
    hdr = b"MATOK" + struct.pack("<HHHHIH", ver, eps, unk, ident, N, s)
    return gzip.compress(hdr + sig + b"M" + out.astype("<u4").tobytes(), 1)


def trie_automaton(triple=False, depth=TRIE_DEPTH):
    """craft._automaton with state 2 ("inside a word") unfolded into a binary trie: word node h (2 = "a", 3 = "b") has
    the children 2h / 2h + 1, the deepest nodes loop to themselves; every node keeps state 2's epsilon and EOT arcs."""
    assert depth >= 2
    base = craft._automaton(triple)
    off, top = max(base), 1 << (depth + 1)
    arcs = {}
    for t, row in base.items():
        if t == 2:
            continue
        r = dict(row)
        for sym, first in ((craft.A, 2), (craft.B, 3)):
            if sym in r and r[sym][0] == 2:
                r[sym] = (off + first, r[sym][1])
        arcs[t] = r
    def word(to_a, to_b):
        return {craft.A: (to_a, False), craft.B: (to_b, False), craft.EPS: base[2][craft.EPS], craft.E: base[2][craft.E]}
    for h in range(2, top):
        ca, cb = (2 * h, 2 * h + 1) if 2 * h + 1 < top else (h, h)
        arcs[off + h] = word(off + ca, off + cb)
    # The ids the unfolding left free (state 2 itself, and off + 0 / off + 1: the trie has no nodes 0 and 1) become word
    # states too, entered from the last node of the deepest level: every id 1..off + top - 1 is a reachable state, so a
    # double array's dense layout has as many states as the matrix (the loader counts what it can reach).
    spare = [t for t in range(1, off + top) if t not in arcs]
    for t in spare:
        arcs[t] = word(t, t)
    last = off + top - 1
    arcs[last] = word(spare[0], spare[-1])
    return arcs


def matok_of(arcs, sigma=None) -> bytes:
    """craft.matok_from for large arc tables (numpy, gzip level 1)."""
    n = max(max(arcs), max(to for row in arcs.values() for to, _ in row.values()))
    s = len(sigma or craft.SIGMA)
    arr = np.zeros((n + 1) * s, dtype=np.uint32)
    for t, row in arcs.items():
        for a, (to, nontoken) in row.items():
            arr[(a - 1) * n + t] = to | (craft.FIRSTBIT if nontoken else 0)
    raw = b"MATOK" + struct.pack("<HHHHIH", 1, craft.EPS, craft.UNKNOWN, craft.IDENTITY, n, s) + craft._sigma_bytes(sigma) + b"M"
    return gzip.compress(raw + arr.astype("<u4").tobytes(), 1)


def datok_of(arcs, sigma=None) -> bytes:
    """A `.datok` image like craft.datok_from's (every arc slot "separate"), with a running base instead of the
    first-fit search, which is quadratic in the states: state t's arcs at base = n + 1 + (t - 1) * s."""
    n = max(max(arcs), max(to for row in arcs.values() for to, _ in row.values()))
    s = len(sigma or craft.SIGMA)
    size = n + 1 + (n + 1) * s
    base = np.zeros(size + s + 2, dtype=np.uint32)
    check = np.zeros(size + s + 2, dtype=np.uint32)
    top = 0
    for t in sorted(arcs):
        b = n + 1 + (t - 1) * s
        base[t] = b
        for a, (to, nontoken) in arcs[t].items():
            base[b + a] = to | craft.FIRSTBIT                       # separate: move on to the representative
            check[b + a] = t | (craft.FIRSTBIT if nontoken else 0)
            top = max(top, b + a)
    check[1] = max(n + 1, top)                                      # datok.go:328-335: the array's size
    pairs = np.empty(2 * len(base), dtype="<u4")
    pairs[0::2], pairs[1::2] = base, check
    raw = (b"DATOK" + struct.pack("<HHHHHHI", 1, craft.EPS, craft.UNKNOWN, craft.IDENTITY, s, s, len(pairs))
           + craft._sigma_bytes(sigma) + b"T")
    return gzip.compress(raw + pairs.tobytes(), 1)


_cache = {}


def trie_model(kind: str, triple=False) -> bytes:
    """The trie tokenizer as a `.matok` / `.datok` image (cached: half a second each)."""
    key = (kind, bool(triple))
    if key not in _cache:
        arcs = trie_automaton(triple)
        _cache[key] = matok_of(arcs) if kind == "matok" else datok_of(arcs)
    return _cache[key]


def word_documents(rng, n_docs, doc_bytes):
    """Running text over craft's alphabet: words of 1..12 letters a / b, blanks, now and then a full stop or a newline."""
    pool = []
    for _ in range(4096):
        k = int(rng.integers(1, 13))
        w = bytes(rng.choice(np.frombuffer(b"ab", dtype=np.uint8), size=k).tolist())
        pool.append(w + (b" ", b" ", b" ", b". ", b"\n")[int(rng.integers(0, 5))])
    per_doc = doc_bytes // 2 + 1             # (a pool entry has at least two bytes)
    docs = []
    for _ in range(n_docs):
        docs.append(b"".join(pool[int(i)] for i in rng.integers(0, len(pool), size=per_doc))[:doc_bytes])
    return docs
