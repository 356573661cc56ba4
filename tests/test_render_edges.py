"""The batch renderer (dtk_batch_render_*, dtk_render.hip) at its own edges: the tiles of RTILE = 1024 scan entries over
the tokens and over the sentence ints (a row has n + 1 entries), the slices of ceil(n / 256) entries that the threads
of the one-block scans over the tile sums and over the documents take, and the bytes that print as U+FFFD beside a tile edge -- in the batch and, at the stream
renderer's tile of 256 tokens, in a stream, since both write such a surface through the same code (sym_expand,
dtk_device.h).  Every batch case compares Batch.render(bits) byte for byte and doc_off entry for entry with the oracle's
transduce of every document."""
import pytest

from streamrender import FFFD, expand_ref, invalid_flags
from test_stream import models  # noqa: F401  (fixture: name -> (device tokenizer, oracle model))
from test_stream_render import assert_rendered

RTILE = 1024
LETTERS = b"abcdefgh"


def words_to_docs(words, counts):
    """The words joined by blanks into len(counts) documents of that many words; no blank behind a document's last."""
    assert sum(counts) == len(words)
    docs, at = [], 0
    for c in counts:
        docs.append(b" ".join(words[at:at + c]))
        at += c
    return docs


def one_letter_words(n):
    return [LETTERS[i % 8:i % 8 + 1] for i in range(n)]


def assert_renders_like_the_oracle(tok, om, docs, modes, totals):
    """Runs the documents as one batch, asserts the totals the case was built for, and compares every mode's bytes and
    document offsets with the oracle's.  Returns the batch's totals."""
    import datok_amd
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    expected = {}
    with datok_amd.Batch(len(text), len(docs)) as b:
        b.set_input(text, off)
        b.run(tok, 0)
        tot = b.totals()
        assert tot["n_flagged"] == 0
        for key, value in totals.items():
            assert tot[key] == value, (key, tot[key], value)
        for bits in modes:
            data, o = b.render(bits)
            at = 0
            for d, doc in enumerate(docs):
                if (doc, bits) not in expected:
                    expected[doc, bits] = om.transduce(doc, bits)
                exp, est = expected[doc, bits]
                assert est == 0
                assert int(o[d]) == at, (bits, d, int(o[d]), at)
                assert data[at:at + len(exp)] == exp, (bits, d, doc[:60], data[at:at + 80], exp[:80])
                at += len(exp)
            assert int(o[len(docs)]) == at == len(data), bits
    return tot


# ---- 1. the tiles over the tokens
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1022, 1023, 1024, 1025])
@pytest.mark.parametrize("name,modes", [("tokenizer_de.matok", tuple(range(16))), ("tokenizer_de.datok", (3, 15))])
def test_token_count_at_the_tile_edge(models, name, modes, n):
    tok, om = models(name)
    docs = words_to_docs(one_letter_words(n), [257, 1, 300, n - 558])
    assert_renders_like_the_oracle(tok, om, docs, modes, {"n_tokens": n})


# ---- 2. the tiles over the sentence ints
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1022, 1024])
def test_sentence_int_count_at_the_tile_edge(models, n):
    """(Every sentence brings its start and its end: a batch has an even number of sentence ints, so rows of 1023 and of
    1025 entries are the two sides of the edge that exist.)"""
    tok, om = models("tokenizer_de.matok")
    sentences = [(b"Ja!", b"Es geht.", b"Nein?")[i % 3] for i in range(n // 2)]
    docs = words_to_docs(sentences, [200, 1, 300, n // 2 - 501])
    assert_renders_like_the_oracle(tok, om, docs, (8, 12, 15), {"n_sent": n})


# ---- 3. the row over the documents
@pytest.mark.gpu
@pytest.mark.parametrize("n_docs", [255, 256, 257, 513])
def test_document_count_at_the_scan_slices(models, n_docs):
    """One short sentence per document (every seventh has two, so that the SentenceEnd counts are no constant): a thread
    of the one-block scan over the documents takes one document up to 256, two from 257 on (the last threads none) and
    three at 513 (the last slice partial)."""
    tok, om = models("tokenizer_de.matok")
    docs = [b"Gut. Ja!" if d % 7 == 3 else (b"Ja!", b"Es geht so.", b"Nein?")[d % 3] for d in range(n_docs)]
    assert_renders_like_the_oracle(tok, om, docs, (2, 3, 15), {"n_texts": n_docs})


# ---- 4. more than 256 token tiles
@pytest.mark.gpu
def test_more_token_tiles_than_scan_threads(models):
    """258 tile sums: slices of two, the upper half of the threads without one."""
    tok, om = models("tokenizer_de.matok")
    counts = [(4001, 3999, 4000)[d % 3] for d in range(66)]
    docs = words_to_docs(one_letter_words(sum(counts)), counts)
    assert sum(counts) + 1 > 256 * RTILE
    assert_renders_like_the_oracle(tok, om, docs, (3, 15), {"n_tokens": sum(counts)})


# ---- 5. bytes that print as U+FFFD beside a tile edge
def sow_invalid(words, edge):
    """Bytes that do not decode in the words `edge` - 2 .. `edge` (those there are): a lone \\xd0 behind a letter, \\xff
    in front of one, \\xff behind one; and an \\xff more as the last byte of all."""
    words = list(words)
    for i, w in ((edge - 2, b"a\xd0"), (edge - 1, b"\xffb"), (edge, b"c\xff")):
        if i < len(words):
            words[i] = w
    words[-1] += b"\xff"
    return words


def invalid_bytes(words):
    return sum(w.count(b"\xff") + w.count(b"\xd0") for w in words)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1023, 1024, 1025])
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.matok:entries", "de64.matok"])
def test_invalid_bytes_beside_the_token_tile_edge(models, name, n):
    """Tokens 1022, 1023 (the last of the first tile) and 1024 carry such a byte, where the batch has them; a document
    in the middle ends in \\xff, and so does the batch."""
    tok, om = models(name)
    words = sow_invalid(one_letter_words(n), RTILE)
    words[299] += b"\xff"
    docs = words_to_docs(words, [300, 1, 400, n - 701])
    assert docs[0].endswith(b"\xff") and docs[-1].endswith(b"\xff")
    assert_renders_like_the_oracle(tok, om, docs, (1, 3, 15), {"n_tokens": n})
    exp = b"".join(om.transduce(doc, 3)[0] for doc in docs)
    assert exp.count(FFFD) == invalid_bytes(words) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_invalid_bytes_beside_the_stream_renderers_tile_edge(models, n):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    words = sow_invalid(one_letter_words(n), 256)
    raw = b" ".join(words)
    assert raw.endswith(b"\xff")
    with datok_amd.Stream(1 << 16) as st:
        for mode in (1, 3):
            slices = assert_rendered(st, tok, om, raw, mode)
            assert len(slices) == 1 and len(slices[0].tok_bend) == n
            assert slices[0].out.count(FFFD) == invalid_bytes(words) >= 2


# ---- 6. the shared byte rule and its capacity, as the tests restate it
def test_expand_rule_stores_nothing_at_or_behind_the_capacity():
    from datok_amd.host import _decode_runes, _runes_to_bytes
    cases = [(b"a\xd0", (0, 1)), (b"\xffb", (1, 0)), (b"c\xff", (0, 1)), (b"\xff\xff", (1, 1)), (b"abc", (0, 0, 0)), (b"", ()),
             ("xä".encode() + b"\xffy", (0, 0, 0, 1, 0)), ("a\ufffd".encode() + b"\xe2\x82", (0, 0, 0, 0, 1, 1))]
    for surface, invalid in cases:
        assert invalid_flags(surface) == [bool(f) for f in invalid]
        full = _runes_to_bytes(_decode_runes(surface))
        assert len(full) == len(surface) + 2 * sum(invalid)
        for o in (0, 5):
            for cap in range(o + len(full) + 3):
                out = bytearray(b"\n" * (o + len(full) + 4))
                assert expand_ref(out, o, surface, invalid, cap) == o + len(full)
                assert out[:o] == b"\n" * o and out[max(cap, o):] == b"\n" * (len(out) - max(cap, o)), (surface, o, cap)
                # in front of the capacity: the full surface, but for a replacement that does not fit whole
                at = o
                for b, bad in zip(surface, invalid):
                    w = 3 if bad else 1
                    want = full[at - o:at - o + w] if at + w <= cap else b"\n" * w
                    assert out[at:at + w] == want, (surface, o, cap, at)
                    at += w


# ---- 7. the shared in-place row scan beyond one round, from its user with the longest rows that a small input reaches
@pytest.mark.gpu
def test_stream_slice_with_more_than_256_token_tiles(models):
    """70 000 tokens in one slice are 274 of the stream renderer's tiles of 256 tokens: scan_row64 (dtk_device.h) takes a
    second round over the tile sums and carries the first round's sum into it."""
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b" ".join(one_letter_words(70000))
    with datok_amd.Stream(1 << 18) as st:
        slices = assert_rendered(st, tok, om, raw, 3)
        assert len(slices) == 1 and len(slices[0].tok_bend) == 70000
