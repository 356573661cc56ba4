"""The batch's readers of the symbol stream where it holds the 16-bit entries themselves (DtkSym with lut == nullptr:
dtk_sym_entry's second branch) and the run saw a byte that does not decode, GPU tier: the key readers of dtk_key.h under
the id lookup, the tally and the WordPiece split at wave and block edges, and the batch renderer of dtk_render.hip in
all 16 writer modes.  The models are bigsigma.device_model's: the shipped automata with the hook SYM16 around their load
and the enlarged model, which has such a stream by itself.  Every comparison is an equality against the plain-Python
definitions (tests/tokenids.py, tests/wordpiece.py) or the oracle's bytes."""
import numpy as np
import pytest

import bigsigma
import symref
import tokenids
import wordpiece
from test_token_ids import REPL, _assert_ids
from test_token_ids import _run as run_ids
from test_wordpiece import _assert_pieces
from test_wordpiece import _run as run_pieces

pytestmark = pytest.mark.gpu

ENTRIES = "tokenizer_de.matok:entries"


@pytest.fixture(scope="module")
def models():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bigsigma.device_model(name)
        return cache[name]
    return get


# ------------------------------------------------------------------------------------ 1: wave and block edges
def _letter_docs(n_tok):
    """n_tok tokens of one letter each, the first and the last with an \\xff appended, in documents with empty ones first,
    last and in runs in the middle: the first token begins at byte 0 of the text, and the text's last byte is the last
    token's \\xff -- a key reader takes the stream's entry of the last byte of the buffer."""
    letters = [bytes([97 + k % 10]) for k in range(n_tok)]
    letters[0] += b"\xff"
    letters[-1] += b"\xff"
    k = max(n_tok // 3, 1)
    docs = [b"", b""]
    for i, part in enumerate([letters[:k], letters[k:2 * k], letters[2 * k:]]):
        if part:
            docs.append(b" ".join(part))
        docs += [b""] * (3 if i < 2 else 2)
    return docs


ID_WORDS = [b"a\xff", b"a", b"c", b"e", b"a" + REPL, b"g", b"i", b"ab", b"", b"\xff", REPL] + [bytes([97 + k]) + REPL for k in range(1, 10)]
WP_WORDS = [b"[UNK]", b"a", b"##\xff", b"##" + REPL, b"c", b"e", b"g", b"i"] + [bytes([97 + k]) for k in (2, 3, 5)]


@pytest.mark.parametrize("device_input", [False, True])
@pytest.mark.parametrize("n_tok", [63, 64, 65, 257])
def test_wave_and_block_edges_with_the_stream_in_use(models, n_tok, device_input):
    """63, 64, 65 and 257 tokens (a wave has 64 lanes, a block 256 threads) with an invalid byte in the batch's first and
    last token, so that every key is read through the stream; host input and a device buffer of exactly `total` bytes.
    Ids, n_unknown and the tally against tests/tokenids.py, the pieces against tests/wordpiece.py."""
    import datok_amd
    tok = models(ENTRIES)[0]
    docs = _letter_docs(n_tok)
    want = [bytes([97 + k % 10]) for k in range(n_tok)]
    want[0] += REPL
    want[-1] += REPL
    vocab = datok_amd.Vocab(ID_WORDS)
    tally = datok_amd.Tally(vocab)
    with datok_amd.Batch(4096, 16) as b:
        ids, n_unknown, r, text, off = run_ids(tok, docs, vocab, batch=b, tally=tally, device_input=device_input)
        assert len(ids) == n_tok and not r.status[np.diff(off.astype(np.int64)) > 0].any()
        keys, exp = _assert_ids(ids, n_unknown, r, text, off, ID_WORDS)
        assert keys == want
        d_of = np.repeat(np.arange(len(docs)), np.diff(r.tok_off.astype(np.int64)))
        assert int(off[d_of[0]]) + int(r.tok_bstart[0]) == 0
        assert int(off[d_of[-1]]) + int(r.tok_bend[-1]) == len(text) and int(text[-1]) == 0xFF
        assert int(ids[0]) == ID_WORDS.index(b"a" + REPL) and int(ids[-1]) == ID_WORDS.index(want[-1])   # never the raw form
        assert 0 < n_unknown < n_tok
        assert np.array_equal(tally.read(), tokenids.expected_counts(ID_WORDS, exp))
        b.set_vocab(None)
        p, r, text, off = run_pieces(tok, docs, datok_amd.Vocab(WP_WORDS), batch=b, device_input=device_input)
        _assert_pieces(p, r, text, off, WP_WORDS)
        assert p.piece_id[:2].tolist() == [1, 3] and p.piece_bend[:2].tolist() == [1, 2]
        last = [i for i, _ in wordpiece.split_key(WP_WORDS, want[-1])[0]]
        assert p.piece_id[-len(last):].tolist() == last and last[-1] == 3 and int(p.piece_bend[-1]) == int(r.tok_bend[-1])
        assert (p.piece_id != 2).all()


# ------------------------------------------------------------------------------------ 2: the batch renderer
INVALID_DOCS = [b"ab\xffcd ef", b"Preis\xe2\x82 hier und \xe2\x82", "ab�cd gut".encode(), b"\xff", b"ganz normal", b"",
                b"x\xc3 y\xf0\x9f\x98 z\x80"]          # (the seven documents of test_wordpiece.py's invalid UTF-8 test)


def _spliced_documents(n=16, size=1024):
    """The first n documents of about `size` bytes of test_stream_render.invalid_stream_spliced, cut at blanks."""
    from test_stream_render import invalid_stream_spliced
    raw, docs, at = invalid_stream_spliced(), [], 0
    while len(docs) < n:
        cut = raw.index(b" ", at + size)
        docs.append(raw[at:cut])
        at = cut + 1
    return docs


_documents = {}


def _render_documents(name):
    if "rows" not in _documents:
        text, what = symref.rows()
        raw = text.tobytes()
        _documents["rows"] = [raw[i * symref.ROW:(i + 1) * symref.ROW] for i in range(len(what))]
    docs = _documents["rows"] + INVALID_DOCS
    return docs + _spliced_documents() if name == "de64.matok" else docs


@pytest.mark.parametrize("name", [ENTRIES, "tokenizer_de.datok:entries", "de64.matok"])
def test_batch_render_in_every_writer_mode(models, name):
    """Every kind of UTF-8 sequence -- well formed, overlong, truncated, stray -- on the symboliser's structural edges
    (symref.rows, one document per row), the invalid documents of the split's test and, for the enlarged model, documents
    with its own characters beside bad bytes: every document's bytes in the 16 writer modes are the oracle's."""
    import datok_amd
    from datok_amd import corpus
    tok, om = models(name)
    docs = _render_documents(name)
    text, off = corpus.concat_docs(docs)
    with datok_amd.Batch(len(text), len(docs)) as b:
        b.set_input(text, off)
        b.run(tok, 0)
        status = b.result().status
        assert [d for d in range(len(docs)) if status[d]] == [docs.index(b"")]       # (an empty text: DTK_ST_EMPTY_TEXT)
        assert int(status[docs.index(b"")]) == datok_amd.ST_EMPTY_TEXT
        for bits in range(16):
            data, o = b.render(bits)
            assert o[0] == 0 and o[-1] == len(data)
            compared = 0
            for d, doc in enumerate(docs):
                exp, est = om.transduce(doc, bits)
                if est and not doc:
                    continue                    # (the reference panics on a text without a token where it prints positions)
                assert est == 0, (bits, d)
                got = data[int(o[d]):int(o[d + 1])]
                if got != exp:
                    k = next((j for j, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
                    raise AssertionError("%s, mode %d, document %d (%r ...): %d bytes against %d, first difference at %d: %r "
                                         "against %r" % (name, bits, d, doc[:24], len(got), len(exp), k,
                                                         got[max(k - 20, 0):k + 20], exp[max(k - 20, 0):k + 20]))
                compared += 1
            assert compared >= len(docs) - 1, bits
