"""The symboliser's reference and corpus (test infrastructure, CPU only).

reference_stream() says what k_symbolize must write for a batch -- one 16-bit entry per input byte, the rune-start
bitmap and the "saw an invalid byte" flag -- from the reference's rules alone: Go's DecodeRune (oracle.decode_rune)
rune by rune inside every document, and the symbol of a rune as matrix.go:421-435 picks it (sigmaASCII below 256, the
sigma map from 256 on, the identity symbol for a miss).  Nothing here is taken from the kernel.

The corpus puts every kind of UTF-8 sequence -- well formed, overlong, surrogate, out of range, stray, truncated --
at every split across the kernel's structural edges: the 512-byte tile, the 1 KiB quarter (one wave, one queue) and
the 4 KiB block staged in LDS with a dword of halo either side.  No random numbers: what a test meets never depends
on where a generator happened to put an umlaut.
"""
import ctypes as C

import numpy as np

W_SHIFT, CLS_SHIFT, SYM_MASK = 11, 14, 0x7FF
BLOCK = 4096
ROW = 3 * BLOCK                                   # a multiple of the block: rows keep their alignment when concatenated
EDGES = (512, 1024, 2048, 4096, 8192)             # tile, quarter, half a block, block, two blocks

SEQUENCES = {
    "well formed": "c3a4 c3bf c480 c280 dfbf e2809e e282ac e697a5 efbfbd e0a080 ed9fbf ee8080 efbfbf "
                   "f0908080 f09f9880 f48fbfbf",
    "in the shipped tokenizers' sigma (the others are not)": "e2809c e280a6",
    "overlong, surrogate or out of range": "c0af c1bf e09fbf eda080 f08fbfbf f4908080 f5808080 ff fe",
    "stray continuations": "80 bf 80808080",
    "truncated": "c3 e2 e282 f0 f09f f09f98",
    "lead followed by ASCII or another lead": "e28241 f09f4180 e2c3a4 f09fe282ac",
    "next to EOT": "e28204 f09f9804",
}
TAILS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 511, 513, 1023, 1025, 4095, 4096, 4097, 4099, 8191)

_WORDS = ("der die und in den von zu das mit sich des auf ist im dem nicht ein Die eine als auch es an werden aus er "
          "hat dass sie nach wird bei einer Der um am sind noch wie einem einen Das so Sie zum war haben nur oder aber "
          "vor zur bis mehr durch man sein wurde sei In Prozent hatte kann gegen vom schon wenn habe seine Mark ihre "
          "dann unter wir soll ich eines Es Jahr zwei Jahren diese dieser wieder keine Uhr seiner worden Und will "
          "zwischen Im immer Millionen Ein was sagte").split()


def sequences(extra=()):
    """The byte sequences of the sweep; extra: more of them (characters of a crafted sigma)."""
    return [bytes.fromhex(h) for hs in SEQUENCES.values() for h in hs.split()] + [bytes(e) for e in extra]


def filler(n):
    """n bytes of ASCII words, every ninth followed by a full stop: single blanks, short tokens, short sentences."""
    out, k = bytearray(), 0
    while len(out) < n:
        out += _WORDS[k % len(_WORDS)].encode()
        k += 1
        out += b". " if k % 9 == 0 else b" "
    return bytes(out[:n])


def rows(extra=()):
    """One ROW-byte row per sequence s and j in 0..len(s): s written at B - j for every B of EDGES, a blank on either
    side -- s lies before, across at every split, and behind each edge.  Returns (uint8 text, [(s, j)] per row)."""
    base = bytearray(filler(ROW))
    base[-1:] = b"\n"
    out, what = [], []
    for s in sequences(extra):
        for j in range(len(s) + 1):
            r = bytearray(base)
            for B in EDGES:
                r[B - j - 1:B - j + len(s) + 1] = b" " + s + b" "
            assert len(r) == ROW
            out.append(bytes(r))
            what.append((s, j))
    return np.frombuffer(b"".join(out), dtype=np.uint8).copy(), what


def layout(n_rows, which, total=None):
    """Document offsets over n_rows rows (or over the first `total` bytes of a text cut loose from the row grid):
    "a" one document per row; "b" documents cut at every B of EDGES: a sequence cut by a document boundary decodes as
    two truncated pieces; "c" a document every 8 bytes: 512 per block, more than the kernel keeps in LDS."""
    total = n_rows * ROW if total is None else total
    if which == "a":
        off = np.arange(0, total + 1, ROW)
    elif which == "b":
        off = (np.arange(n_rows)[:, None] * ROW + np.array((0,) + EDGES)[None, :]).ravel()
        off = np.append(off, total)
    else:
        off = np.arange(0, total + 8, 8)
        off[-1] = total
        if len(off) > 1 and off[-2] == total:
            off = off[:-1]
    return off.astype(np.uint64)


def tail(n):
    """A batch of n bytes for the ragged end: 0x80 first and a truncated e2 82 last, as far as n bytes hold both (the
    end wins at two bytes)."""
    t = bytearray(filler(n))
    t[0:1] = b"\x80"
    if n >= 2:
        t[-2:] = b"\xe2\x82"
    return np.frombuffer(bytes(t), dtype=np.uint8).copy(), np.array([0, n], dtype=np.uint64)


def dense():
    """Queues filled to their 1024 entries: 512 x c3a4 on a quarter edge, 1024 x 80, 4096 x ff, each a document of
    its own between two documents of words, and the same bytes one byte further on.  Returns (text, doc_off)."""
    parts, off = [], [0]
    for payload in (b"\xc3\xa4" * 512, b"\x80" * 1024, b"\xff" * 4096):
        for shift in (0, 1):
            head = filler(1024 + shift)
            size = -(-(len(head) + len(payload) + 1) // BLOCK) * BLOCK
            for piece in (head, payload, filler(size - len(head) - len(payload))):
                parts.append(piece)
                off.append(off[-1] + len(piece))
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64)


def empty_runs():
    """Words with runs of 70 and of 4100 empty documents immediately before and immediately behind the byte at each
    4096 boundary, and at both ends of a batch with a ragged last block.  Returns (text, doc_off)."""
    total = 3 * BLOCK + 5
    text = np.frombuffer(filler(total), dtype=np.uint8).copy()
    # offset -> empty documents there (offset B: between byte B - 1 and byte B; B + 1: right behind byte B)
    cuts = {0: 4100, BLOCK: 70, BLOCK + 1: 4100, 2 * BLOCK: 4100, 2 * BLOCK + 1: 70, 3 * BLOCK: 70, 3 * BLOCK + 1: 70,
            total: 4100}
    off = [0]
    for at in sorted(cuts):
        if at > off[-1]:
            off.append(at)                     # the document of words that ends here
        off += [at] * cuts[at]
    assert off[-1] == total
    return text, np.array(off, dtype=np.uint64)


# ------------------------------------------------------------------ the reference
def decode_stream(text, doc_off):
    """(rune, width) per input byte: Go's DecodeRune rune by rune inside every document (an invalid byte: U+FFFD,
    width 1); width 0 and rune 0 where no rune starts.  Bytes below 0x80 are runes of their own whatever surrounds
    them (numpy); only the maximal runs of bytes >= 0x80 are walked rune by rune, each decode seeing the document's
    bytes behind the run too."""
    from oracle import oracle as O
    text = np.ascontiguousarray(text, dtype=np.uint8)
    off = np.asarray(doc_off).astype(np.int64)
    n = int(off[-1])
    assert off[0] == 0 and n == len(text) and np.all(np.diff(off) >= 0)
    rune = np.where(text < 0x80, text, 0).astype(np.uint32)
    width = (text < 0x80).astype(np.uint8)
    hi = np.flatnonzero(text >= 0x80)
    if len(hi) == 0:
        return rune, width
    brk = np.flatnonzero(np.diff(hi) > 1)
    run_s = hi[np.concatenate(([0], brk + 1))]
    run_e = hi[np.concatenate((brk, [len(hi) - 1]))] + 1
    raw = text.tobytes()
    for s, e in zip(run_s.tolist(), run_e.tolist()):
        i, dend = s, -1
        while i < e:
            if i >= dend:                       # the document of byte i (empty documents own no byte)
                dend = int(off[np.searchsorted(off, i, side="right")])
            r, w = O.decode_rune(raw[i:min(i + 4, dend)])
            assert 1 <= w <= dend - i
            rune[i], width[i] = r, w
            i += w
    return rune, width


def reference_stream(omodel, text, doc_off):
    """(entries uint16[total], starts bool[total], saw_invalid) for a batch, from the model file alone.
    entries: symbol | width << 11 | class << 14 (include/datok_gpu.h, dtk_batch_debug_stream); where no rune starts
    the width field is 0 and nothing else of the entry is defined."""
    from oracle import oracle as O
    rune, width = decode_stream(text, doc_off)
    text = np.asarray(text, dtype=np.uint8)
    ascii_sym = np.asarray(omodel.sigma_ascii()).astype(np.uint32)
    identity = omodel.info["identity"]
    miss = 0 if identity < 0 else identity      # a net without an identity symbol: a map miss leaves a == 0
    sym = np.zeros(len(text), dtype=np.uint32)
    cls = np.zeros(len(text), dtype=np.uint32)
    low = (width > 0) & (rune < 256)
    sym[low] = ascii_sym[rune[low]]
    cls[low & (rune == 4)] = 1
    ok = C.c_int(0)
    for i in np.flatnonzero((width > 0) & (rune >= 256)).tolist():
        a = O.lib().orc_sigma_lookup(omodel._h, int(rune[i]), C.byref(ok))
        sym[i], cls[i] = (a, 2) if ok.value else (miss, 3)
    assert int(sym.max(initial=0)) <= SYM_MASK
    entries = (sym | (width.astype(np.uint32) << W_SHIFT) | (cls << CLS_SHIFT)).astype(np.uint16)
    entries[width == 0] = 0
    saw_invalid = bool(np.any((width == 1) & (text >= 0x80)))
    return entries, width > 0, saw_invalid


def pack_bits(starts):
    """bool[total] -> uint32[(total + 31) // 32], bit g of the array = byte g."""
    b = np.packbits(np.asarray(starts, dtype=bool), bitorder="little")
    b = np.concatenate((b, np.zeros(-len(b) % 4, dtype=np.uint8)))
    return b.view("<u4").astype(np.uint32)


def doc_of(doc_off, pos):
    """The document that owns byte `pos`."""
    return int(np.searchsorted(np.asarray(doc_off).astype(np.int64), pos, side="right")) - 1


def assert_stream_equal(got, ref, text, doc_off, what=""):
    """got: Batch.debug_stream() -> (entries, rune_start_words, saw_invalid); ref: reference_stream().  Every byte of
    every document: the width field everywhere, the whole entry where a rune starts, every bit of the bitmap (none set
    at or behind `total`), and the flag.  A failure names the first byte position and its document."""
    g_ent, g_words, g_flag = got
    r_ent, r_starts, r_flag = ref
    total = len(r_ent)
    assert len(g_ent) == total and len(g_words) == (total + 31) // 32, (what, len(g_ent), len(g_words), total)
    g_ent, r_ent = np.asarray(g_ent, dtype=np.uint16), np.asarray(r_ent, dtype=np.uint16)

    def fail(kind, pos, g, r):
        d = doc_of(doc_off, pos)
        a, b = max(int(doc_off[d]), pos - 6), min(int(doc_off[d + 1]), pos + 6)
        raise AssertionError("%s: %s differs at byte %d of document %d (byte %d of the batch): got %s, reference %s; "
                             "bytes %d..%d of the batch: %s" % (what, kind, pos - int(doc_off[d]), d, pos, g, r, a, b,
                                                              bytes(np.asarray(text[a:b], dtype=np.uint8)).hex()))
    bad = np.flatnonzero((g_ent >> W_SHIFT & 7) != (r_ent >> W_SHIFT & 7))
    if len(bad):
        p = int(bad[0])
        fail("width", p, int(g_ent[p]) >> W_SHIFT & 7, int(r_ent[p]) >> W_SHIFT & 7)
    bad = np.flatnonzero(r_starts & (g_ent != r_ent))
    if len(bad):
        p = int(bad[0])
        fail("entry (symbol, width, class)", p, (int(g_ent[p]) & SYM_MASK, int(g_ent[p]) >> W_SHIFT & 7, int(g_ent[p]) >> CLS_SHIFT),
             (int(r_ent[p]) & SYM_MASK, int(r_ent[p]) >> W_SHIFT & 7, int(r_ent[p]) >> CLS_SHIFT))
    g_bits = np.unpackbits(np.asarray(g_words, dtype="<u4").view(np.uint8), bitorder="little").astype(bool)
    bad = np.flatnonzero(g_bits[:total] != r_starts)
    if len(bad):
        p = int(bad[0])
        fail("rune-start bit", p, int(g_bits[p]), int(r_starts[p]))
    assert not g_bits[total:].any(), "%s: rune-start bits set at or behind the batch's %d bytes" % (what, total)
    assert bool(g_flag) == bool(r_flag), "%s: saw_invalid is %s, the reference says %s" % (what, g_flag, r_flag)
