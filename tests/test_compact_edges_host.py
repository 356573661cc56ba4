"""The documents of compactedges.py hold what their names say -- pinned on the CPU oracle, so that the GPU tests of
test_compact_edges.py cannot become vacuous: every token, EOT and sentence end sits at the cursor position the
compaction kernels' structure makes interesting (tile 2048, word 32, step 256, round 64, ring and row stage 512)."""
import numpy as np
import pytest

import compactedges as ce
from compactedges import NEWLINE_AFTER_EOT, TILE

MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")
EMPTY_TEXT = 2


@pytest.fixture(scope="module")
def om(oracle_models):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ce.CachedOracle(oracle_models(name))
        return cache[name]
    return get


def tokens(r):
    return set(zip((int(x) for x in r.tok_bstart), (int(x) for x in r.tok_bend)))


@pytest.mark.parametrize("model", MODELS_DE)
@pytest.mark.parametrize("flags", [0, NEWLINE_AFTER_EOT])
def test_status_of_every_family(om, model, flags):
    """Oracle status 0 for every document of every family, on both encodings and both flag values, except the named
    ones: the empty documents (A2's prefix of 0 bytes, A5's first and last) and A4's texts without a token carry
    EMPTY_TEXT; A1 is the edge-document list of test_gpu_parity.py with its window overflows and invalid bytes, of
    which most are in contract."""
    o = om(model)

    def status(docs):
        return [o.transduce_doc(d, flags).status for d in docs]
    for name, fn in list(ce.A_FAMILIES.items()) + list(ce.B_FAMILIES.items()) + [("A5", ce.a5_mixed)]:
        st = status(fn())
        if name == "A1":
            assert sum(s == 0 for s in st) > 350 and len(st) > 400
        elif name == "A2":
            assert st[0] == EMPTY_TEXT and not any(st[1:])
        elif name == "A4":
            assert st == [c[1] for c in ce.A4_CASES]
        elif name == "A5":
            assert st[0] == st[-1] == EMPTY_TEXT and not any(st[1:-1])
        else:
            assert not any(st), (name, [i for i, s in enumerate(st) if s][:5])


def test_window_limits_the_families_stay_below(om):
    """A run of more than about 1000 blanks overflows the window (status 1), one of 1000 does not; B5's longest run is
    900 blanks and B2's longest token 1000 runes."""
    o = om("tokenizer_de.matok")
    assert o.transduce_doc(b"Satz." + b" " * 2100 + b"Neu.").status == 1
    assert o.transduce_doc(b"Satz." + b" " * 1000 + b"Neu.").status == 0
    assert o.transduce_doc(b"x" * 1100).status == 1
    assert max(ce.B5_BLANKS) <= 1000


@pytest.mark.parametrize("model", MODELS_DE)
def test_a2_a_call_at_the_last_positions_for_every_length_modulo_32(om, model):
    """Among the prefixes, for every residue of len modulo 32 one document has a token that ends at len and one a token
    that ends at len - 1; the text holds runes of two, three and four bytes, an EOT with a newline, and prefixes that
    end inside a rune."""
    o = om(model)
    at_len, below = set(), set()
    for d in ce.a2_prefixes():
        ends = set(int(x) for x in o.transduce_doc(d).tok_bend)
        if len(d) in ends:
            at_len.add(len(d) % 32)
        if len(d) - 1 in ends:
            below.add(len(d) % 32)
    assert at_len == set(range(32)) and below == set(range(32)), (sorted(at_len), sorted(below))
    t = ce.A2_TEXT[:ce.A2_MAX]
    s = t.decode("utf-8", "ignore")
    assert {len(c.encode()) for c in s} == {1, 2, 3, 4} and b"\x04\n" in t and b". " in t
    assert [len(d) for d in ce.a2_prefixes()] == list(range(ce.A2_MAX + 1))
    bad = 0
    for d in ce.a2_prefixes():
        try:
            d.decode()
        except UnicodeDecodeError:
            bad += 1
    assert bad >= 10
    assert len(o.transduce_doc(t).text_tok_end) == 2


@pytest.mark.parametrize("model", MODELS_DE)
def test_a3_tokens_over_word_edges(om, model):
    """Every case's token is one token of the oracle's, 30..34 or 62..66 bytes long; the ends fall one below, at and
    one above a word edge, the starts one, two and three words before the end's word; half are written as two-byte
    runes (rune length != byte length)."""
    o = om(model)
    spans, wide = set(), 0
    for d, s, e in ce.a3_cases():
        r = o.transduce_doc(d)
        assert (s, e) in tokens(r), (s, e, d)
        assert e - s in ce.A3_LENGTHS
        i = list(r.tok_bend).index(e)
        wide += int(r.tok_rend[i] - r.tok_rstart[i]) < e - s
        spans.add((e % 32, e // 32 - s // 32))
    assert {x for x, _ in spans} == {31, 0, 1}
    assert {1, 2, 3} <= {w for _, w in spans}
    assert all((x, 1) in spans and (x, 2) in spans for x in (31, 0, 1))
    assert wide == len(ce.a3_cases()) // 2


def test_a4_the_newline_rule_shows(om):
    """EOT first, last, doubled; behind `\\x04\\n` a token's offsets differ between the two flag values (the rule moves
    the text's origin behind the newline), on the matrix."""
    o = om("tokenizer_de.matok")
    docs = ce.a4_eot_placements()
    assert docs[0][0] == 4 and docs[1][-1] == 4 and b"\x04\x04" in docs[3] and b"\n" in docs
    d = docs[4]
    a, b = o.transduce_doc(d, 0), o.transduce_doc(d, NEWLINE_AFTER_EOT)
    assert len(a.text_tok_end) == 2 and not np.array_equal(a.tok_rstart, b.tok_rstart)
    assert np.array_equal(a.tok_bstart, b.tok_bstart)
    d = b"\nHallo Welt."       # no text has ended: the rule does not fire for a document's first token
    assert np.array_equal(o.transduce_doc(d, 0).tok_rstart, o.transduce_doc(d, NEWLINE_AFTER_EOT).tok_rstart)
    assert d in docs


def test_a5_sizes_around_the_limit():
    docs = ce.a5_mixed()
    lens = [len(d) for d in docs]
    assert lens[0] == lens[-1] == 0
    assert {159, 160, 161, 5000} <= set(lens) and ce.A5_SMALL_MAX == 160
    big = [i for i, n in enumerate(lens) if n > 160]
    assert sum(n == 5000 for n in lens) == 4 and any(b"\x04" in docs[i] for i in big if lens[i] == 5000)
    assert all(lens[i - 1] in (159, 160, 161) and lens[i + 1] in (159, 160, 161) for i in big if lens[i] == 5000)
    assert any(d.endswith(b"\x04") and len(d) == 160 for d in docs)


@pytest.mark.parametrize("model", MODELS_DE)
def test_b1_last_positions_of_a_tile(om, model):
    """Every length 2040..2056 and 4090..4100 with each ending; a document that ends in a token has its last token end
    at len -- for len = 2048 and 4096 the END bit is the only position of the last tile; the EOT ending closes a
    text."""
    o = om(model)
    docs = ce.b1_lengths()
    assert sorted({len(d) for d in docs}) == list(ce.B1_LENGTHS) and len(docs) == 4 * len(ce.B1_LENGTHS) + 1
    assert {2047, 2048, 2049, 4095, 4096, 4097} <= set(ce.B1_LENGTHS)
    for i, d in enumerate(docs[:-1]):
        r = o.transduce_doc(d)
        e = ce.B1_ENDINGS[i % 4]
        assert d.endswith(e)
        if e == b"":
            assert int(r.tok_bend[-1]) == len(d)
        elif e == b". ":
            assert int(r.tok_bend[-1]) == len(d) - 1
        elif e == b"\x04":
            assert int(r.tok_bend[-1]) == len(d) - 1 and len(r.text_tok_end) == 1 and r.status == 0
        else:
            assert int(r.tok_bend[-1]) == len(d) - 1
    d = docs[-1]
    r = o.transduce_doc(d)
    assert len(d) == 2048 and (2044, 2048) in tokens(r) and r.status == 0


@pytest.mark.parametrize("model", MODELS_DE)
def test_b2_tokens_across_position_2048(om, model):
    """A token with bstart = 2048 - k and bend >= 2048 exists for every k in 1..40, one with bend = 2048 + j for every
    j in 1..40; runes of more than one byte stand before each (rune index < byte index); the token of 1000 `日` spans
    (2025, 5025)."""
    o = om(model)
    ks, js = set(), set()
    for d, s, e in ce.b2_cases():
        r = o.transduce_doc(d)
        assert (s, e) in tokens(r), (s, e)
        i = list(r.tok_bend).index(e)
        if e - s < 100:
            assert int(r.tok_rstart[i]) < s
            assert s < TILE < e
            ks.add(TILE - s)
            js.add(e - TILE)
    assert ks == set(range(1, 41)) and js == set(range(1, 41))
    d, s, e = ce.b2_cases()[-1]
    assert (s, e) == (2025, 5025) and s < TILE and e > 2 * TILE
    assert {(k, j) for k in (32, 33) for j in (1, 32, 33)} <= set(ce.b2_sweep())


@pytest.mark.parametrize("model", MODELS_DE)
def test_b3_more_tokens_in_a_tile_than_staged_rows(om, model):
    o = om(model)
    docs = ce.b3_dense()
    r = o.transduce_doc(docs[0])
    assert int((r.tok_bend < TILE).sum()) == 1024 > ce.CT_CAP
    for d, tile in zip(docs[1:], (0, 0, 1)):
        r = o.transduce_doc(d)
        in_tile = (r.tok_bend >= tile * TILE) & (r.tok_bend < (tile + 1) * TILE)
        assert int(in_tile.sum()) > ce.CT_CAP + 64, int(in_tile.sum())
        assert len(d) > (tile + 1) * TILE + 600 and int((r.tok_bend >= (tile + 1) * TILE).sum()) > 100
    for d in docs[2:]:      # sentence ends among the rows behind the staged ones
        r = o.transduce_doc(d)
        assert len(r.sent) >= 2 * 320


@pytest.mark.parametrize("model", MODELS_DE)
def test_b4_eot_placements(om, model):
    """eot_at(p) has its EOT at byte p and two texts; b4_queued(n) has n + 1 tokens before its EOT, 63, 64 and 65 among
    them; the dense documents hold more than 512 calls in the tile of their EOT."""
    o = om(model)
    for p in ce.B4_EOT_AT + (3000,):
        d = ce.eot_at(p)
        assert len(d) == 6000 and d[p] == 4 and d.count(b"\x04") == 1
        r = o.transduce_doc(d)
        assert len(r.text_tok_end) == 2 and r.status == 0
    assert TILE < 3000 < 2 * TILE and {255, 256, 257, 2047, 2048, 2049} <= set(ce.B4_EOT_AT)
    before = [int(o.transduce_doc(ce.b4_queued(n)).text_tok_end[0]) for n in ce.B4_QUEUED]
    assert before == [n + 1 for n in ce.B4_QUEUED] and {63, 64, 65} <= set(before) and {63, 64, 65} <= set(ce.B4_QUEUED)
    assert all(ce.b4_queued(n).find(b"\x04") < ce.STEP for n in ce.B4_QUEUED)
    docs = ce.b4_eot_tiles()
    assert all(len(d) > 2 * TILE for d in docs)
    dense = [d for d in docs if b"c c c c" in d]
    assert len(dense) == 2
    for d in dense:
        p = d.find(b"\x04")
        t0 = p // TILE * TILE
        r = o.transduce_doc(d)
        assert int(((r.tok_bend >= t0) & (r.tok_bend < t0 + TILE)).sum()) > ce.CQ_CAP + 2 * ce.ROUND
    assert [d.find(b"\x04") // TILE for d in dense] == [0, 1]
    every = docs[-1 - len(ce.b4_far_cases())]
    assert sorted(i // TILE for i, c in enumerate(every) if c == 4) == [0, 1, 2]
    for d, spans in ce.b4_far_cases():     # long tokens in the EOT's tile, one of them across position 2048
        r = o.transduce_doc(d)
        p = d.find(b"\x04")
        assert set(spans) <= tokens(r) and r.status == 0
        assert all(e - s > 32 and (e - 1) // TILE == p // TILE for s, e in spans)
    assert sum(s < TILE < e for _, spans in ce.b4_far_cases() for s, e in spans) == 2


@pytest.mark.parametrize("model", MODELS_DE)
def test_b5_the_sentence_latch(om, model):
    """"Satz." ends at `at`, "Neu" starts k bytes later and -- from one blank on -- starts a sentence; each run length
    once inside tile 0, once across position 2048 and once ending there."""
    o = om(model)
    seen = set()
    for d, at in ce.b5_cases():
        r = o.transduce_doc(d)
        i = list(r.tok_bend).index(at)
        k = int(r.tok_bstart[i + 1]) - at
        assert d[at - 5:at] == b"Satz." and d[at + k:at + k + 4] == b"Neu." and d[at:at + k] == b" " * k
        assert int(r.tok_bend[i + 1]) == at + k + 3
        if k >= 1:
            assert int(r.tok_rstart[i + 1]) in set(int(x) for x in r.sent)
        where = ("starts" if at == TILE else "ends" if at + k == TILE else "across" if at < TILE < at + k else
                 "inside" if at + k + 4 < TILE else "other")
        seen.add((k, where))
    for k in ce.B5_BLANKS:
        assert (k, "inside") in seen, k
        if k >= 2:
            assert (k, "across") in seen and (k, "ends") in seen, k
    assert (0, "starts") in seen and (1, "ends") in seen


def test_production_batch_has_the_lane_kernels_shape(om):
    """What dtk_run.cpp asks before it launches k_compact_small by itself, and what the pool mixes in."""
    pieces, pick = ce.production_batch()
    lens = np.array([len(pieces[i]) for i in pick])
    assert len(pick) >= ce.LANE_MIN_DOCS and int((lens <= ce.LANE_SMALL_BYTES).sum()) >= ce.LANE_MIN_SMALL
    assert int((lens > ce.LANE_SMALL_BYTES).sum()) >= 200
    pool = ce.small_pool()
    assert len(set(pool)) >= 2500 and all(len(p) <= ce.LANE_SMALL_BYTES for p in pool)
    assert {len(p) % 32 for p in pool} == set(range(32))
    assert sum(b"\x04" in p for p in pool) > 500 and sum(b"\x04\n" in p for p in pool) > 100
    assert sum(any(c >= 0x80 for c in p) for p in pool) > 1000
    o = om("tokenizer_de.matok")
    st = [o.transduce_doc(p).status for p in pool]
    assert sum(s == 0 for s in st) > 0.95 * len(pool) and set(st) <= {0, EMPTY_TEXT}
