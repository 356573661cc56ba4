"""Documents at the compaction's structural edges, and the checks that go with them (test infrastructure).

dtk_compact.hip writes every array a caller reads from the walk's event bitmaps, in three implementations of
NewTokenWriter: the wave kernels' fast tile path, the queued heavy rounds of k_compact_eot, and k_compact_small with
one lane per document.  Their structure -- tiles of 2048 cursor positions over len + 1 positions, 32 positions per
lane, steps of 256, heavy rounds of 64 queued positions, a ring and a row stage of 512 entries, a backward search for
tokens of more than 32 bytes, words and latches handed from tile to tile -- shows in no result, so the documents here
are built around those numbers: the A-families for the lane kernel (everything is sent through it with the hook
SMALL_MAX), the B-families for the wave kernels (SMALL_MAX = 0).

Both kernel families end with "did my counts fill the rows the walk sized?" and hand a document that does not add up
to the exact pass (k_exact_doc), which then writes correct rows: a compaction that loses a call only makes the run
slow.  check() therefore looks at BatchResult.exact as well -- see exact_rule().

The builders are pure functions that return lists of bytes; tests/test_compact_edges_host.py pins on the oracle that
each family holds what its name says.
"""
import contextlib

import numpy as np

from parity import FIELDS, assert_batch_equals_oracle

TOKENS, SENTENCES, TOKEN_POS, SENTENCE_POS, NEWLINE_AFTER_EOT = 1, 2, 4, 8, 16
SIMPLE = TOKENS | SENTENCES

TILE = 2048        # cursor positions of a wave kernel's tile (32 per lane, 64 lanes)
WORD = 32          # positions per lane / per bitmap word
STEP = 256         # positions queued per light step of a heavy tile
ROUND = 64         # queued positions per heavy round
CQ_CAP = 512       # ring capacity in queued positions
CT_CAP = 512       # rows of a fast tile staged in LDS
# dtk_run.cpp, the block that sets b->small_max: the lane kernel runs for a batch of at least LANE_MIN_DOCS documents
# of which at least LANE_MIN_SMALL are at most LANE_SMALL_BYTES long
LANE_MIN_DOCS, LANE_MIN_SMALL, LANE_SMALL_BYTES = 2048, 16384, 160

ROW_ARRAYS = ("tok_off", "sent_off", "text_off", "status") + FIELDS


# ------------------------------------------------------------------------------------------------ hook and runs
@contextlib.contextmanager
def small_max(n):
    """The hook SMALL_MAX: documents of at most n bytes go to the lane kernel, whatever the batch's shape (0: none).
    Read when a batch plans its input -- plan_lanes() in dtk_run.cpp, called by the first run after set_input -- and
    a batch keeps its plan for equally shaped input: every setting gets a fresh Batch, with the hook around set_input
    and that run."""
    import datok_amd
    configure = datok_amd.lib().dtk_debug_configure
    assert configure(b"SMALL_MAX", str(int(n)).encode()) == 0
    try:
        yield
    finally:
        assert configure(b"SMALL_MAX", b"-1") == 0


@contextlib.contextmanager
def ran(tok, docs, flags=0, sm=None, chunking=None):
    """A fresh batch that has run `docs`: yields (batch, res, text, off).  sm: SMALL_MAX for this batch (None: the
    library decides by shape); chunking: None for one lane per document, else (chunk, warm)."""
    import datok_amd
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    with datok_amd.Batch(max(len(text), 1), len(docs)) as b:
        if chunking is None:
            b.set_chunking(0, 64)
        elif chunking != "auto":
            b.set_chunking(chunking[0], chunking[1])
        with (small_max(sm) if sm is not None else contextlib.nullcontext()):
            b.set_input(text, off)
            b.run(tok, flags)
        yield b, b.result(), text, off


class CachedOracle:
    """The oracle's answers per distinct (document, flags), computed once (what parity.py and check() ask for)."""

    def __init__(self, model):
        self.model, self.info = model, model.info
        self._doc, self._out = {}, {}

    def transduce_doc(self, doc, flags=0):
        k = (doc, flags)
        if k not in self._doc:
            self._doc[k] = self.model.transduce_doc(doc, flags)
        return self._doc[k]

    def transduce(self, doc, flags=SIMPLE):
        k = (doc, flags)
        if k not in self._out:
            self._out[k] = self.model.transduce(doc, flags)
        return self._out[k]


def exact_rule(is_matrix, flags):
    """True: no document the oracle accepts may come from the exact pass.  That holds for a matrix model without
    NEWLINE_AFTER_EOT: its calls are in position order and neither kernel family has a case it leaves to the exact
    pass.  The double array fires an EOT's calls out of position order (datok.go:1019-1030) and NEWLINE_AFTER_EOT has
    the "token that ends at offset 0" case (dtk_compact.hip): there the walk or the wave kernels hand documents over
    by design, and the rule is relative -- the lane kernel hands over no document that the wave kernels keep."""
    return is_matrix and not (flags & NEWLINE_AFTER_EOT)


def check(om, batch, res, text, off, flags, expect_exact=None):
    """Every field and the status against the oracle, the rendered bytes of two writer modes (which read tok_sbefore,
    text_s_end and doc_ns), and the exact pass: expect_exact None -- no document with oracle status 0 in res.exact;
    a set -- res.exact holds no document outside it.  Returns the number of documents compared field by field."""
    n_docs = len(off) - 1
    raw = text.tobytes()
    docs = [raw[int(off[d]):int(off[d + 1])] for d in range(n_docs)]
    n = assert_batch_equals_oracle(om, res, text, off, flags)
    ok = [d for d in range(n_docs) if om.transduce_doc(docs[d], flags).status == 0]
    assert n == len(ok)
    for bits in (SIMPLE, 15):
        data, o = batch.render(bits | flags)
        assert o[0] == 0 and o[-1] == len(data)
        for d in ok:
            exp, est = om.transduce(docs[d], bits | flags)
            assert est == 0
            got = data[int(o[d]):int(o[d + 1])]
            assert got == exp, ("rendered", bits | flags, d, docs[d][:80], got[:120], exp[:120])
    exact = set(int(d) for d in res.exact)
    if expect_exact is None:
        bad = sorted(exact & set(ok))
        assert not bad, ("left to the exact pass", bad[:8], [docs[d][:60] for d in bad[:3]])
    else:
        bad = sorted(exact - set(expect_exact))
        assert not bad, ("left to the exact pass by this run only", bad[:8], [docs[d][:60] for d in bad[:3]])
    return n


def assert_same_rows(a, b):
    for f in ROW_ARRAYS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and np.array_equal(x, y), f


def check_lane_and_wave(tok, om, docs, flags, sm=4096, chunking=None):
    """`docs` once through the wave kernels (SMALL_MAX 0) and once with every document of at most sm bytes through
    the lane kernel, each on a fresh batch: both equal the oracle, the rows of the two runs are equal array for
    array, and the exact pass gets what exact_rule() allows.  Returns (wave exact set, lane exact set)."""
    strict = exact_rule(om.info["kind"] == 0, flags)
    # (the first batch stays open while the second runs: a batch that is freed hands its device memory, rows of the
    #  same documents included, to the next one of the same shape -- a kernel that writes nothing would go unnoticed)
    with ran(tok, docs, flags, sm=0, chunking=chunking) as (b, wave, text, off):
        check(om, b, wave, text, off, flags, expect_exact=None if strict else set(range(len(docs))))
        with ran(tok, docs, flags, sm=sm, chunking=chunking) as (b2, lane, text, off):
            check(om, b2, lane, text, off, flags, expect_exact=None if strict else set(int(d) for d in wave.exact))
    assert_same_rows(wave, lane)
    return set(int(d) for d in wave.exact), set(int(d) for d in lane.exact)


# ------------------------------------------------------------------------------------------------ building blocks
WORDS = ["der", "alte", "Mann", "ging", "über", "die", "Straße", "und", "sah", "ein", "Haus", "am", "See", "später",
         "kam", "Regen", "日本", "heute", "früh", "noch", "Zeit", "für", "Bücher", "im", "Garten"]


def filler(n, shift=0):
    """Exactly n bytes of ordinary German words with a sentence end every seventh word; ends in a letter (the last
    word is padded with x), holds runes of two and three bytes, no blank-free run beyond a few dozen bytes."""
    out, i = bytearray(), shift
    while True:
        w = WORDS[i % len(WORDS)].encode() + (b"." if i % 7 == 6 else b"") + b" "
        if len(out) + len(w) + 1 > n:
            break
        out += w
        i += 1
    return bytes(out) + b"x" * (n - len(out))


def filler_blank(n, shift=0):
    """n bytes of filler that end in a blank (n >= 2)."""
    return filler(n - 1, shift) + b" "


def letters(n, wide):
    """A blank-free token of n bytes: plain letters, or written as `ä`s (an odd n starts with one plain letter)."""
    return b"q" * n if not wide else b"q" * (n % 2) + "ä".encode() * (n // 2)


# ------------------------------------------------------------------------------------------------ A: the lane kernel
def a1_edge_docs():
    """The edge documents of test_gpu_parity.py (empty, ragged, EOT, invalid UTF-8, window overflows)."""
    from test_gpu_parity import _edge_docs
    return _edge_docs()


A2_TEXT = ("Ärger ob 日本 😀 da. Ja\x04\nEs ist „so“. im am nie hier, an zu tat er es, tun war, so, da uns Tag wo, oft, an, Ort, "
           "ob sein, es je, ja, noch da, uns, am nie ").encode()
A2_MAX = 160


def a2_prefixes():
    """Every prefix of 0..160 bytes of one text with runes of two, three and four bytes, a sentence end and an EOT
    followed by a newline; its short words and commas put a call at len and one at len - 1 for every length modulo 32
    (a prefix that ends inside a rune ends in invalid bytes)."""
    assert len(A2_TEXT) >= A2_MAX
    return [A2_TEXT[:n] for n in range(A2_MAX + 1)]


A3_LENGTHS = (30, 31, 32, 33, 34, 62, 63, 64, 65, 66)
A3_ENDS = (63, 64, 65, 95, 96, 97, 127, 128, 129)


def a3_cases():
    """(document, token start, token end): one token of 30..34 or 62..66 bytes, plain and as `ä`s, that ends one
    below, at and one above a 32-position word edge and starts one or two words earlier."""
    out = []
    for wide in (False, True):
        for n in A3_LENGTHS:
            for e in A3_ENDS:
                s = e - n
                if s < 3:
                    continue
                out.append((filler_blank(s) + letters(n, wide) + b" und Ende.", s, e))
    return out


def a3_long_tokens():
    return [c[0] for c in a3_cases()]


# (document, oracle status on tokenizer_de): 2 = EMPTY_TEXT, a TextEnd or SentenceEnd in a text without a token
A4_CASES = [
    (b"\x04Hallo Welt.", 2),                       # EOT at byte 0
    (b"Hallo Welt.\x04", 0),                       # EOT as the last byte
    (b"Hallo Welt\x04", 0),
    (b"Hallo.\x04\x04Welt.", 2),                   # two EOTs in a row
    (b"Hallo.\x04\nWelt geht.", 0),                # EOT, newline, token
    (b"Hallo.\x04\n\nWelt geht.", 0),
    (b"Hallo.\x04\nW", 0),
    (b"Hallo.\x04Welt geht.\x04\nDrei.", 0),
    ("Ärger.\x04\nÜber uns.\x04\nÖl.".encode(), 0),
    (b"\nHallo Welt.", 0),                         # a first token behind a newline: no text has ended yet
    (b"\n", 2),                                    # a single newline
    (b"\x04", 2),
    (b"\x04\n", 2),
]


def a4_eot_placements():
    return [c[0] for c in A4_CASES]


A5_SMALL_MAX = 160


def a5_mixed():
    """For SMALL_MAX = 160: documents of 159, 160 and 161 bytes around documents of 5000 bytes (one of them with an EOT
    text), an empty document first and last -- both kernel families write into one set of arrays, the wave kernels from
    the list of the larger documents."""
    big = filler(5000, 3)
    big_eot = filler(2600, 5) + b".\x04\n" + filler(2397, 9)
    docs = [b""]
    for shift in range(4):
        docs += [filler(159, shift), filler(160, shift), filler(161, shift), big if shift % 2 == 0 else big_eot,
                 filler(161, shift + 4), filler(160, shift + 4)[:-1] + b"\x04", filler(159, shift + 4)]
    return docs + [b""]


# ------------------------------------------------------------------------------------------------ B: the wave kernels
B1_LENGTHS = tuple(range(2040, 2057)) + tuple(range(4090, 4101))
B1_ENDINGS = (b"", b". ", b"\x04", b"\n")


def b1_lengths():
    """Documents of 2040..2056 and 4090..4100 bytes that end in a token, in a sentence end and a blank, in an EOT and
    in a newline: the last cursor position (len) is the last of a tile, the only one of the next, or near either."""
    return [filler(n - len(e), n) + e for n in B1_LENGTHS for e in B1_ENDINGS] + [(b"ab cd. " * 400)[:2045] + b"xyz"]


def b2_sweep():
    """(k, j): the token starts k bytes before position 2048 and ends j bytes behind it."""
    ks = [(k, j) for k in range(1, 41) for j in (1, 31, 32, 33, 40)]
    js = [(k, j) for j in range(1, 41) for k in (1, 32, 33, 40)]
    return sorted(set(ks + js))


def b2_cases():
    """(document, token start, token end): a token over position 2048 -- up to 32 bytes before it the start comes from
    the previous tile's last word, beyond that from the backward search -- plain and, where its length is even, as
    `ä`s; two-byte runes stand before it.  And one token of 1000 three-byte runes that starts in tile 0, covers tile 1
    and ends in tile 2."""
    out = []
    for k, j in b2_sweep():
        for wide in (False, True):
            if wide and (k + j) % 2:
                continue
            out.append((filler_blank(TILE - k, k) + letters(k + j, wide) + b" danach kam Regen.", TILE - k, TILE + j))
    out.append((b"Vor. " * 405 + "日".encode() * 1000 + b" nach.", 2025, 5025))
    return out


def b2_straddle():
    return [c[0] for c in b2_cases()]


def b3_dense():
    """More tokens in a tile than rows are staged in LDS: 1024 tokens end below position 2048; the same with a
    sentence end every third token (tok_sbefore is not zero in the rows that go out directly); ordinary text in the
    next tile."""
    tail = b" " + filler(700, 2) + b"."
    return [b"a " * 1100, b"a " * 1100 + tail, b"Da ja! " * 320 + tail, filler_blank(TILE, 1) + b"Da ja! " * 320 + tail]


B4_EOT_AT = (254, 255, 256, 257, 258, 2046, 2047, 2048, 2049, 2050)
B4_QUEUED = (62, 63, 64, 65, 66)


def eot_at(p, n=6000):
    """A document of n bytes whose byte p is an EOT (behind a sentence end, before a newline)."""
    return filler(p - 1, p) + b".\x04\n" + filler(n - p - 2, p + 1)


def b4_queued(n):
    """n tokens of one letter, one more token and an EOT right behind it: n + 1 positions are queued before the
    EOT's."""
    return b"a " * n + b"b\x04\n" + filler(5000, n)


def b4_far_cases():
    """(document, [(token start, token end)]): tokens of more than 32 bytes in a tile that also holds an EOT -- the
    heavy path has its own copy of the previous-word lookup and of the backward search -- inside the tile and across
    position 2048."""
    q, w = letters, "ä".encode()
    return [
        (filler(90, 1) + b".\x04\n" + q(70, False) + b" " + w * 20 + b" " + q(100, False) + b" Ende. " + filler(4200, 2),
         [(93, 163), (164, 204), (205, 305)]),
        (filler_blank(TILE - 20, 3) + q(50, False) + b" und.\x04\n" + q(70, True) + b" Ende. " + filler(2100, 4),
         [(TILE - 20, TILE + 30), (TILE + 37, TILE + 107)]),
        (filler_blank(TILE - 40, 5) + q(60, False) + b" und.\x04\n" + filler(2100, 6), [(TILE - 40, TILE + 20)]),
    ]


def b4_eot_tiles():
    """Three-tile documents: an EOT in the middle tile only (fast, heavy, fast); an EOT at and around the step edge 256
    and the tile edge 2048; 63, 64 and 65 positions queued before an EOT (a heavy round holds 64); a dense tile with an
    EOT, first and second tile (more than 512 positions queued in one tile: the ring wraps); EOTs in every tile; long
    tokens in tiles with an EOT (b4_far_cases)."""
    docs = [eot_at(3000)]
    docs += [eot_at(p) for p in B4_EOT_AT]
    docs += [b4_queued(n) for n in B4_QUEUED]
    dense = b"a " * 700 + b"b.\x04\n" + b"c " * 300
    docs += [dense + filler(4000, 1), filler_blank(TILE, 2) + dense + filler(2000, 3)]
    docs += [filler(1000, 1) + b".\x04\n" + filler(2000, 2) + b"\x04" + filler(2000, 3) + b".\x04\n" + filler(900, 4)]
    return docs + [c[0] for c in b4_far_cases()]


B5_BLANKS = (0, 1, 30, 31, 32, 33, 63, 64, 65, 900)


def b5_cases():
    """(document, position of the sentence's last byte): "Satz.", k blanks, "Neu." -- the pending sentence start is a
    latch set by the SentenceEnd and reset by the next token's end, k + 4 positions later: inside one tile, with the
    run of blanks across position 2048, and with the run ending at 2048."""
    out = []
    for k in B5_BLANKS:
        for at in (300, TILE - k // 2, TILE - k):    # first blank (or, without one, the N of "Neu.")
            if at < 40:
                continue
            head = filler_blank(at - 5, k) + b"Satz."
            assert len(head) == at
            out.append((head + b" " * k + b"Neu. " + filler(60, k) + b".", at))
    return out


def b5_latch():
    return [c[0] for c in b5_cases()]


A_FAMILIES = {"A1": a1_edge_docs, "A2": a2_prefixes, "A3": a3_long_tokens, "A4": a4_eot_placements}
B_FAMILIES = {"B1": b1_lengths, "B2": b2_straddle, "B3": b3_dense, "B4": b4_eot_tiles, "B5": b5_latch}


# ------------------------------------------------------------------------------------------------ the production shape
def small_pool(n_pieces=3000, seed=17):
    """A few thousand distinct pieces of at most 160 bytes: German text cut on rune boundaries into pieces of 1..160
    bytes (every length modulo 32), some with an EOT and a newline put in, some ending in an EOT."""
    from datok_amd import corpus
    raw = corpus.german_docs(64, 4096, seed=seed)[0].tobytes()
    rng = np.random.default_rng(seed)
    pieces, p = [], 0
    while len(pieces) < n_pieces:
        q = p + int(rng.integers(1, 156))
        while (raw[q] & 0xC0) == 0x80:      # (at most three bytes further)
            q += 1
        d = raw[p:q]
        p = q
        how = len(pieces) % 8
        if how == 3 and len(d) > 8:
            cut = len(d) // 2
            while (d[cut] & 0xC0) == 0x80:
                cut += 1
            d = d[:cut] + (b"\x04\n" if len(pieces) % 16 == 3 else b"\x04") + d[cut:]
        elif how == 6:
            d = d + b"\x04"
        pieces.append(d)
    assert all(len(d) <= LANE_SMALL_BYTES for d in pieces)
    return pieces


def production_batch(seed=23, n_small=17500, n_large=300):
    """(documents, piece index per document): n_small documents drawn from small_pool() and n_large larger ones (200
    bytes .. 5 KiB of filler, every third with an EOT text), shuffled."""
    rng = np.random.default_rng(seed)
    pool = small_pool()
    large = []
    for i in range(n_large):
        n = int(rng.integers(200, 5000))
        large.append(filler(n, i) if i % 3 else filler(n // 2, i) + b".\x04\n" + filler(n - n // 2, i + 1))
    pieces = pool + large
    pick = np.concatenate([rng.integers(0, len(pool), size=n_small), len(pool) + np.arange(n_large)])
    rng.shuffle(pick)
    return pieces, pick
