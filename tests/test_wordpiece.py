"""Every token split into WordPiece ids on the device (dtk_batch_set_wordpiece of include/datok_gpu.h), GPU tier: the
kernels of dtk_wordpiece.hip and their plumbing through batch, pipeline and stream.  The delivered piece_off, piece_id,
piece_bend and both counters equal the definition of tests/wordpiece.py applied to the SAME run's delivered tok_bstart /
tok_bend / tok_off and text.  The result is exact: every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest

import bigsigma
import streamcorpus
import tokenids
import wordpiece
from test_event_list import _pipeline_documents
from test_token_ids import MODELS_ENTRIES, DeviceInput, _from_device, _runtime
from wordpiece import FAMILIES, REPL, family_ids

NO_BYTE_OFFSETS = 512
MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")


@pytest.fixture(scope="module")
def gpu():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache = {}

    def get(name):
        """name: a fixture file, "<file>:entries" for its stream as 16-bit entries, or "de64.matok" (bigsigma.device_model)"""
        if name not in cache:
            cache[name] = bigsigma.device_model(name)[0]
        return cache[name]
    return get


def _B():
    import datok_amd
    return datok_amd.Batch


def _assert_pieces(p, r, text, off, words, prefix=b"##", unk_id=0, max_runes=0):
    """A Pieces against the definition on the same run's delivered rows; returns the expected arrays."""
    e_off, e_id, e_bend, e_unknown = wordpiece.expected_pieces(words, text, off, r.tok_off, r.tok_bstart, r.tok_bend,
                                                               prefix, unk_id, max_runes)
    assert p.piece_off.dtype == np.uint64 and p.piece_id.dtype == np.int32 and p.piece_bend.dtype == np.uint32
    assert np.array_equal(p.piece_off, e_off), (p.piece_off[:8], e_off[:8], len(p.piece_off), len(e_off))
    bad = np.flatnonzero(p.piece_id != e_id) if p.piece_id.shape == e_id.shape else None
    assert bad is not None and not len(bad), (bad[:4], p.piece_id[bad[:4]], e_id[bad[:4]])
    bad = np.flatnonzero(p.piece_bend != e_bend)
    assert not len(bad), (bad[:4], p.piece_bend[bad[:4]], e_bend[bad[:4]])
    assert p.n_pieces == len(e_id) == int(e_off[-1]) and p.n_unknown == e_unknown
    return e_off, e_id, e_bend, e_unknown


class _PointerAttributes(C.Structure):
    """hipPointerAttribute_t (with room behind it, should the runtime's be longer)."""
    _fields_ = [("type", C.c_int), ("device", C.c_int), ("devicePointer", C.c_void_p), ("hostPointer", C.c_void_p),
                ("isManaged", C.c_int), ("allocationFlags", C.c_uint), ("room", C.c_uint64 * 8)]


def _memory_type(ptr):
    """What kind of memory the runtime says `ptr` points into (hipMemoryType, as a number)."""
    h = _runtime()
    h.hipPointerGetAttributes.argtypes = [C.POINTER(_PointerAttributes), C.c_void_p]
    a = _PointerAttributes()
    assert h.hipPointerGetAttributes(C.byref(a), C.c_void_p(ptr)) == 0, ptr
    return int(a.type)


def _assert_device_view(v, host):
    """A device view's arrays lie in device memory -- the kind hipMalloc hands out -- whether or not pieces_home has
    brought a copy home, and nowhere near the host view's page-locked ones."""
    h = _runtime()
    probe = C.c_void_p()
    assert h.hipMalloc(C.byref(probe), 64) == 0
    try:
        device_kind = _memory_type(probe.value)
    finally:
        assert h.hipFree(probe) == 0
    for name in ("piece_off", "piece_id", "piece_bend"):
        ptr, arr = getattr(v, name), getattr(host, name)
        assert ptr and _memory_type(ptr) == device_kind, (name, _memory_type(ptr), device_kind)
        if len(arr):
            assert _memory_type(arr.ctypes.data) != device_kind, name
            assert not (arr.ctypes.data <= ptr < arr.ctypes.data + arr.nbytes), name


def _device_pieces(b):
    """The device view, copied back; its pointers are device pointers."""
    import datok_amd
    v = b.pieces(device=True)
    _assert_device_view(v, b.pieces(copy=False))
    return datok_amd.Pieces(_from_device(v.piece_off, int(v.n_tok) + 1, np.uint64), _from_device(v.piece_id, int(v.n_pieces), np.int32),
                            _from_device(v.piece_bend, int(v.n_pieces), np.uint32), int(v.n_pieces), int(v.n_unknown))


def _same(p, q):
    return (np.array_equal(p.piece_off, q.piece_off) and np.array_equal(p.piece_id, q.piece_id) and
            np.array_equal(p.piece_bend, q.piece_bend) and (p.n_pieces, p.n_unknown) == (q.n_pieces, q.n_unknown))


def _run(tok, docs, vocab, batch=None, prefix=b"##", unk_id=0, max_runes=0, pieces_home=True, device_input=False, flags=0):
    """(Pieces, BatchResult, text, doc_off) of one run with the split attached."""
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    b = batch or _B()(max(len(text), 1), len(docs))
    dev = None
    try:
        if device_input:
            dev = DeviceInput(text, off)
            b.set_input_device(dev.text.value, dev.off.value, len(docs), len(text), keep=dev, doc_off_host=off)
        else:
            b.set_input(text, off)
        b.set_wordpiece(vocab, prefix=prefix, unk_id=unk_id, max_runes=max_runes, pieces_home=pieces_home)
        b.run(tok, flags)
        r = b.result()
        p = b.pieces()
        assert len(p.piece_off) == b.totals()["n_tokens"] + 1
        assert _same(_device_pieces(b), p)
        return p, r, text, off
    finally:
        if batch is None:
            b.close()
        if dev is not None:
            dev.close()


def _token_index(r, text, off, key):
    keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)
    assert key in keys, key
    return keys.index(key)


# --------------------------------------------------------------------------------------- 1: the word families
@pytest.mark.gpu
@pytest.mark.parametrize("pieces_home", [True, False])
@pytest.mark.parametrize("model", MODELS_DE)
def test_families_in_german_documents(gpu, model, pieces_home):
    """Every family's keys as tokens of small German documents, one run per family on ONE batch: each run has another
    vocabulary and some another prefix, so every run but the first is a second run on the same batch."""
    import datok_amd
    tok = gpu(model)
    with _B()(4096, 8) as b:
        for name, words, prefix, cases in FAMILIES:
            keys = [k for k, _ in cases if k]
            docs = [b"Der " + k + b" ist da." for k in keys] + [b"", b"Und " + b" und ".join(keys) + b" auch"]
            vocab = datok_amd.Vocab(words)
            p, r, text, off = _run(tok, docs, vocab, batch=b, prefix=prefix, pieces_home=pieces_home)
            _assert_pieces(p, r, text, off, words, prefix)
            for key, expected in cases:
                if not key:
                    continue
                i = _token_index(r, text, off, key)
                a, z = int(p.piece_off[i]), int(p.piece_off[i + 1])
                assert p.piece_id[a:z].tolist() == family_ids(words, expected), (name, key)
                assert int(p.piece_bend[z - 1]) == int(r.tok_bend[i])               # the last piece ends where the token does
            assert p.n_unknown >= sum(1 for k, e in cases if k and e is None) + 4   # ("Der", "ist", "da", ".": no family has them)


# -------------------------------------------------------------------------------------------- 2: invalid UTF-8
@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS_DE + MODELS_ENTRIES)
def test_invalid_utf8_and_source_byte_spans(gpu, model):
    """A lone 0xFF, a truncated E2 82 and a literal U+FFFD inside tokens: a replaced byte is one source byte and three
    key bytes, and piece_bend counts source bytes.  The same batch then runs valid text."""
    import datok_amd
    tok = gpu(model)
    words = [b"[UNK]", b"ab", b"##" + REPL, b"##cd", REPL, b"Preis", b"x", b"y", b"z", b"##" + REPL + REPL, b"ef", b"hier",
             b"##\xff", b"##\xe2\x82", b"g", b"##ut"]
    docs = [b"ab\xffcd ef", b"Preis\xe2\x82 hier und \xe2\x82", "ab�cd gut".encode(), b"\xff", b"ganz normal", b"",
            b"x\xc3 y\xf0\x9f\x98 z\x80"]
    with _B()(4096, 8) as b:
        p, r, text, off = _run(tok, docs, datok_amd.Vocab(words), batch=b)
        _assert_pieces(p, r, text, off, words)
        keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)
        i = keys.index(b"ab" + REPL + b"cd")                          # document 0: ab FF cd, source bytes 0..5
        assert int(r.tok_off[0]) == i and (int(r.tok_bstart[i]), int(r.tok_bend[i])) == (0, 5)
        assert p.piece_id[int(p.piece_off[i]):int(p.piece_off[i + 1])].tolist() == [1, 2, 3]
        assert p.piece_bend[int(p.piece_off[i]):int(p.piece_off[i + 1])].tolist() == [2, 3, 5]
        j = keys.index(b"ab" + REPL + b"cd", i + 1)                   # document 2: the literal U+FFFD, three source bytes
        assert p.piece_id[int(p.piece_off[j]):int(p.piece_off[j + 1])].tolist() == [1, 2, 3]
        assert p.piece_bend[int(p.piece_off[j]):int(p.piece_off[j + 1])].tolist() == [2, 5, 7]
        k = keys.index(b"Preis" + REPL + REPL)                        # the truncated sequence: two replaced bytes, one piece
        assert p.piece_id[int(p.piece_off[k]):int(p.piece_off[k + 1])].tolist() == [5, 9]
        assert p.piece_bend[int(p.piece_off[k]):int(p.piece_off[k + 1])].tolist() == [5, 7]
        assert (p.piece_id != 12).all() and (p.piece_id != 13).all()  # no raw form matched
        valid = [b"ganz normal und gut", b"ab cd ef hier x"]
        p, r, text, off = _run(tok, valid, datok_amd.Vocab(words), batch=b)
        _assert_pieces(p, r, text, off, words)
        assert 14 in p.piece_id and 15 in p.piece_id and 0 < p.n_unknown < len(p.piece_off) - 1


@pytest.mark.gpu
def test_invalid_utf8_beside_the_letters_of_an_enlarged_model(gpu):
    """bigsigma.enlarged_de(64), whose stream holds 16-bit entries by itself: pieces that end and begin at a replaced
    byte beside the new two-byte letters.  A replaced byte is one source byte; the raw forms are in the vocabulary and
    never match."""
    import datok_amd
    l = [x.encode() for x in bigsigma.LETTERS[:5]]
    words = [b"[UNK]", l[0] + l[1], b"##" + REPL, b"##" + l[2] + l[3], REPL, b"Preis", b"##" + l[0] + REPL, l[1] + REPL,
             b"##" + l[2], b"x", b"z", b"##" + REPL + l[4], l[4], b"##" + REPL + REPL, b"ef", b"hier",
             b"##\xff", b"##" + l[0] + b"\xd0", l[1] + b"\xd0", b"\xff", b"##\xf0\x9f\x98"]
    n_replaced_forms = 16
    docs = bigsigma.invalid_documents()
    with _B()(4096, 8) as b:
        p, r, text, off = _run(gpu("de64.matok"), docs, datok_amd.Vocab(words), batch=b)
        _assert_pieces(p, r, text, off, words)
        keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)

        def pieces(key, start=0):
            i = keys.index(key, start)
            a, z = int(p.piece_off[i]), int(p.piece_off[i + 1])
            return i, p.piece_id[a:z].tolist(), p.piece_bend[a:z].tolist()
        whole = l[0] + l[1] + REPL + l[2] + l[3]
        i, ids, bend = pieces(whole)                                  # document 0: two letters, FF, two letters: source bytes 0..9
        assert (int(r.tok_bstart[i]), int(r.tok_bend[i])) == (0, 9) and (ids, bend) == ([1, 2, 3], [4, 5, 9])
        j, ids, bend = pieces(whole, i + 1)                           # document 3: the literal U+FFFD, three source bytes
        assert (ids, bend) == ([1, 2, 3], [4, 7, 11])
        assert pieces(b"Preis" + l[0] + REPL)[1:] == ([5, 6], [5, 8])  # a piece that ends in the lone lead byte
        assert pieces(l[1] + REPL)[1] == [7]
        assert pieces(REPL + l[2] + REPL)[1:] == ([4, 8, 2], [1, 3, 4])   # one letter between two replaced bytes
        k, ids, bend = pieces(b"z" + REPL + l[4])
        assert ids == [10, 11] and bend[1] - bend[0] == 3
        assert pieces(l[4] + 3 * REPL)[1] == [12, 13, 2]
        assert (p.piece_id < n_replaced_forms).all()                  # no raw form matched


# ------------------------------------------------------------------------------- 3: block and scan-tile edges
def _a_docs(n_tok):
    """n_tok tokens -- 1 to 7 times "a", or "x" -- in documents with empty ones first, last and in runs in the middle:
    the first token begins at byte 0 of the text and the last one ends at its last byte."""
    toks = [b"x" if k % 11 == 10 else b"a" * (1 + k % 7) for k in range(n_tok)]
    k = max(n_tok // 3, 1)
    docs = [b"", b""]
    for i, part in enumerate([toks[:k], toks[k:2 * k], toks[2 * k:]]):
        if part:
            docs.append(b" ".join(part))
        docs += [b""] * (3 if i < 2 else 2)
    return docs


A_WORDS = [b"[UNK]", b"a", b"##a", b"##aaa"]    # 1 to 7 times "a": 1, 2, 3, 2, 3, 4, 3 pieces


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_block_and_tile_edges(gpu, device_input):
    """1, 255, 256 and 257 tokens in a batch (a block and a scan tile have 256 lanes) with one to four pieces each, with
    equal neighbours in tok_off, and batches without a token; host input and a device buffer of exactly `total` bytes
    whose last byte is the last token's."""
    import datok_amd
    vocab = datok_amd.Vocab(A_WORDS)
    tok = gpu(MODELS_DE[0])
    with _B()(8192, 16) as b:
        for n_tok in (1, 255, 256, 257):
            docs = _a_docs(n_tok)
            p, r, text, off = _run(tok, docs, vocab, batch=b, device_input=device_input)
            assert len(p.piece_off) == n_tok + 1 and not r.status[np.diff(off.astype(np.int64)) > 0].any(), n_tok
            _assert_pieces(p, r, text, off, A_WORDS)
            d_of = np.repeat(np.arange(len(docs)), np.diff(r.tok_off.astype(np.int64)))
            assert int(off[d_of[0]]) + int(r.tok_bstart[0]) == 0
            assert int(off[d_of[-1]]) + int(r.tok_bend[-1]) == len(text)          # the last piece ends at the text's last byte
            assert int(p.piece_bend[-1]) == int(r.tok_bend[-1])
            counts = np.diff(p.piece_off.astype(np.int64))
            assert counts.min() == 1 and (n_tok < 255 or (counts.max() == 4 and p.n_unknown == n_tok // 11))
        for docs in ([b"", b"  ", b""], [b""]):
            p, r, text, off = _run(tok, docs, vocab, batch=b, device_input=device_input)
            assert p.piece_off.tolist() == [0] and p.n_pieces == 0 and p.n_unknown == 0 and len(p.piece_id) == 0


@pytest.mark.gpu
def test_many_tokens_and_a_block_that_grows(gpu):
    """About 70 000 tokens of 1 to 4 pieces over 274 scan tiles: more than twice as many pieces as tokens, so the run is
    split a second time into a block that holds them; the next, small run on the same batch is right again."""
    import datok_amd
    vocab = datok_amd.Vocab(A_WORDS)
    tok = gpu(MODELS_DE[0])
    docs = _a_docs(70001)
    with _B()(1 << 19, 16) as b:
        p, r, text, off = _run(tok, docs, vocab, batch=b, pieces_home=False)
        assert len(p.piece_off) == 70002 and p.n_pieces > 2 * 70001
        _assert_pieces(p, r, text, off, A_WORDS)
        q = b.pieces(copy=False)                                       # a second call hands out the same block
        assert _same(p, q)
        p, r, text, off = _run(tok, _a_docs(300), vocab, batch=b)
        _assert_pieces(p, r, text, off, A_WORDS)


@pytest.mark.gpu
def test_one_token_of_a_hundred_pieces(gpu):
    """100 times "a" over a and ##a: 100 pieces, each one byte further; 101 times is too long and unknown."""
    import datok_amd
    words = [b"[UNK]", b"a", b"##a"]
    tok = gpu(MODELS_DE[0])
    with _B()(1024, 2) as b:
        p, r, text, off = _run(tok, [b"a" * 100], datok_amd.Vocab(words), batch=b)
        assert len(r.tok_bend) == 1
        _assert_pieces(p, r, text, off, words)
        assert p.piece_id.tolist() == [1] + [2] * 99 and p.piece_bend.tolist() == list(range(1, 101)) and p.n_unknown == 0
        p, r, text, off = _run(tok, [b"a" * 101, b"a" * 5], datok_amd.Vocab(words), batch=b)
        _assert_pieces(p, r, text, off, words)
        assert p.piece_id.tolist() == [0, 1, 2, 2, 2, 2] and p.piece_bend.tolist() == [101, 1, 2, 3, 4, 5] and p.n_unknown == 1
        p, r, text, off = _run(tok, [b"a" * 101, b"a" * 5], datok_amd.Vocab(words), batch=b, max_runes=4)
        assert p.piece_id.tolist() == [0, 0] and p.piece_bend.tolist() == [101, 5] and p.n_unknown == 2


# ------------------------------------------------------------------- 4: a vocabulary and a split side by side
@pytest.mark.gpu
def test_vocabulary_and_split_together(gpu):
    """Ids over one vocabulary, pieces over another, a tally: both are right, asking for either in any order changes
    nothing, and the tally counts each token once.  Then a second run with another prefix, unk_id and vocabulary."""
    import datok_amd
    from datok_amd import corpus
    tok = gpu(MODELS_DE[0])
    docs = _pipeline_documents()[:6] + [b"", b"der die das der"]
    surfaces = sorted({w for d in docs for w in d.split()})
    id_words = surfaces[::2] + [b",", b"."]
    heads = sorted({s[:3] for s in surfaces})
    wp_words = [b"[UNK]", b",", b"."] + heads + sorted({b"##" + s[k:k + 2] for s in surfaces for k in range(3, len(s), 2)})
    id_vocab, wp_vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(wp_words)
    tally = datok_amd.Tally(id_vocab)
    text, off = corpus.concat_docs(docs)
    with _B()(1 << 16, 16) as b:
        b.set_input(text, off)
        b.set_vocab(id_vocab, tally=tally)
        b.set_wordpiece(wp_vocab)
        b.run(tok, 0)
        p = b.pieces()
        ids, n_unknown = b.token_ids()
        r = b.result()
        _assert_pieces(p, r, text, off, wp_words)
        keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)
        exp = tokenids.expected_ids(id_words, keys)
        assert np.array_equal(ids, exp) and n_unknown == int((exp < 0).sum())
        assert (np.diff(p.piece_off.astype(np.int64)) > 1).sum() > 100 and 0 < p.n_unknown
        b.pieces(); b.token_ids(); b.download_begin(); b.result(); b.pieces(device=True)
        assert np.array_equal(tally.read(), tokenids.expected_counts(id_words, exp))
        assert _same(b.pieces(), p) and np.array_equal(b.token_ids()[0], ids)
        # the same input again: another vocabulary, prefix and unk_id for the split; the ids stay
        other = [w.replace(b"##", b"+") for w in wp_words[1:]] + [b"<unk>"]
        b.set_wordpiece(datok_amd.Vocab(other), prefix=b"+", unk_id=len(other) - 1)
        b.run(tok, 0)
        q = b.pieces()
        _assert_pieces(q, b.result(), text, off, other, b"+", len(other) - 1)
        assert np.array_equal(q.piece_off, p.piece_off) and q.n_unknown == p.n_unknown
        assert np.array_equal(b.token_ids()[0], ids)
        assert np.array_equal(tally.read(), 2 * tokenids.expected_counts(id_words, exp))


# --------------------------------------------------------------------------------------------------- 5: errors
@pytest.mark.gpu
def test_errors(gpu):
    import datok_amd
    from datok_amd import _lib, corpus
    tok = gpu(MODELS_DE[0])
    vocab = datok_amd.Vocab([b"[UNK]", b"a", b"##b"])

    def code(fn, *a, **kw):
        with pytest.raises(_lib.DatokGpuError) as e:
            fn(*a, **kw)
        return e.value.code
    text, off = corpus.concat_docs([b"a ab c", b"", b"abb"])
    with _B()(1024, 4) as b:
        for device in (False, True):
            assert code(b.pieces, device=device) == _lib.E_STATE                  # before a run, without a split
        b.set_wordpiece(vocab)
        assert code(b.pieces) == _lib.E_STATE                                     # before a run
        b.set_input(text, off)
        b.run(tok, 0)
        assert b.pieces().piece_id.tolist() == [1, 1, 2, 0, 1, 2, 2] and b.pieces().n_unknown == 1
        for bad in (dict(unk_id=3), dict(unk_id=-1), dict(prefix=b"#" * 17)):
            assert code(b.set_wordpiece, vocab, **bad) == _lib.E_ARG              # rejected on the host, and nothing changes
        assert b.pieces().piece_off.tolist() == [0, 1, 3, 4, 7]
        b.set_wordpiece(None)
        assert code(b.pieces) == _lib.E_STATE                                     # without a split
        b.set_vocab(vocab)
        assert code(b.pieces) == _lib.E_STATE                                     # (a vocabulary alone is no split)
        b.set_vocab(None)
        b.set_wordpiece(vocab, max_runes=2)
        assert b.pieces().piece_id.tolist() == [1, 1, 2, 0, 0]                    # the finished run, split under the new rule
        b.run(tok, NO_BYTE_OFFSETS)
        for device in (False, True):
            assert code(b.pieces, device=device) == _lib.E_STATE                  # the keys are cut out with the byte offsets
        assert len(b.result().tok_rstart) == 4                                    # (the other results come as before)
        b.run(tok, 0)
        assert b.pieces().piece_id.tolist() == [1, 1, 2, 0, 0]
        assert datok_amd.lib().dtk_batch_pieces_host(b._h, None) == _lib.E_ARG
    with datok_amd.Stream(16384) as s:
        v = _lib.PieceView()
        assert datok_amd.lib().dtk_stream_pieces(s._h, C.byref(v)) == _lib.E_STATE   # outside slice_fn
        assert code(s.set_wordpiece, vocab, unk_id=3) == _lib.E_ARG
    with datok_amd.Pipeline(32 << 10, 16) as p:
        assert code(p.set_wordpiece, vocab, prefix=b"#" * 17) == _lib.E_ARG
        p.set_wordpiece(vocab)
        p.set_wordpiece(None)


# ------------------------------------------------------------------------------------------------ 6: pipeline
def _corpus_vocab(raw_words):
    """A vocabulary that splits a real share of running text: every third surface whole, the first three bytes of the
    others as first pieces, and continuation pieces of two bytes and of one."""
    surfaces = sorted(set(raw_words))
    rest = [s for k, s in enumerate(surfaces) if k % 3]
    conts = {b"##" + s[k:k + 2] for s in rest[::2] for k in range(3, len(s), 2)} | {b"##" + s[k:k + 1] for s in rest[::5] for k in range(3, len(s))}
    words = [b"[UNK]", b",", b"."] + surfaces[::3] + sorted({s[:3] for s in rest}) + sorted(conts)
    return [w for w in words if _valid(w)]


def _valid(w):
    try:
        w.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.gpu
@pytest.mark.parametrize("fields", [True, False])
def test_pipeline(gpu, fields):
    """64 documents of 2-6 KB in ragged slices of 32 KB, depth 3: the slices' pieces joined are the pieces of the same
    documents as one batch -- with result fields on the pipeline (the pieces come home with the slice) and without."""
    import datok_amd
    B = _B()
    tok = gpu(MODELS_DE[0])
    docs = _pipeline_documents()
    words = _corpus_vocab([w for d in docs for w in d.split()])
    vocab = datok_amd.Vocab(words)
    p1, r, text, off = _run(tok, docs, vocab)
    _assert_pieces(p1, r, text, off, words)
    counts = np.diff(p1.piece_off.astype(np.int64))
    assert (counts > 1).sum() > 1000 and 0 < p1.n_unknown < len(counts)
    got = []

    def on_slice(first, n, b):
        p = b.pieces()
        assert len(p.piece_off) == b.totals()["n_tokens"] + 1
        got.append(p)
    with datok_amd.Pipeline(32 << 10, 64, depth=3) as p:
        p.set_wordpiece(vocab, pieces_home=fields)
        if fields:
            p.set_result_fields(B.R_CSR | B.R_STATUS)
        p.run(tok, text, off, 0, on_slice)
        assert len(got) >= 6
        assert np.array_equal(np.concatenate([g.piece_id for g in got]), p1.piece_id)
        assert np.array_equal(np.concatenate([g.piece_bend for g in got]), p1.piece_bend)
        assert np.array_equal(np.concatenate([np.diff(g.piece_off.astype(np.int64)) for g in got]), counts)
        assert sum(g.n_unknown for g in got) == p1.n_unknown and sum(g.n_pieces for g in got) == p1.n_pieces
        p.run(tok, text, off, NO_BYTE_OFFSETS, None)                   # a run without byte offsets has no pieces


# -------------------------------------------------------------------------------------------------- 7: stream
@pytest.mark.gpu
@pytest.mark.parametrize("pieces_home", [True, False])
def test_stream(gpu, pieces_home):
    """64 KB of German text at Stream(16384): the slices' pieces joined are the pieces of the same text as one document,
    with piece_bend relative to each slice's window like its tok_bend."""
    import datok_amd
    tok = gpu(MODELS_DE[0])
    raw = streamcorpus.construct_stream("token300", 0) + b" " + streamcorpus.running_text(24 << 10, seed=11)
    words = [w for w in _corpus_vocab(raw.split()) if w != b"a" * 300] + [b"a" * 100, b"##" + b"a" * 100]
    vocab = datok_amd.Vocab(words)
    p1, r, text, off = _run(tok, [raw], vocab, max_runes=300)
    _assert_pieces(p1, r, text, off, words, max_runes=300)
    counts = np.diff(p1.piece_off.astype(np.int64))
    assert not r.status.any() and (counts > 1).sum() > 500 and 0 < p1.n_unknown < len(counts)
    long_tok = int(np.flatnonzero(r.tok_bend.astype(np.int64) - r.tok_bstart.astype(np.int64) == 300)[0])
    assert counts[long_tok] == 3                                       # the token of 300 "a": three pieces of 100
    slices = []
    with datok_amd.Stream(streamcorpus.S) as s:
        s.set_wordpiece(vocab, max_runes=300, pieces_home=pieces_home)
        assert s.run(tok, raw, 0, slices.append) == 0
        streamcorpus.check_slices(slices, len(raw))
        assert len(slices) >= 3
        assert sum(sl.n_pieces for sl in slices) == p1.n_pieces and sum(sl.n_piece_unknown for sl in slices) == p1.n_unknown
        if pieces_home:
            assert all(len(sl.piece_off) == len(sl.tok_bend) + 1 and int(sl.piece_off[0]) == 0 for sl in slices)
            assert np.array_equal(np.concatenate([sl.piece_id for sl in slices]), p1.piece_id)
            assert np.array_equal(np.concatenate([np.diff(sl.piece_off.astype(np.int64)) for sl in slices]), counts)
            # (piece_bend is relative to the slice's window like tok_bend; the window begins at stream byte `base`)
            ends = np.concatenate([sl.piece_bend.astype(np.int64) + sl.base for sl in slices])
            assert np.array_equal(ends, p1.piece_bend.astype(np.int64))
        else:
            assert all(sl.piece_off is None and sl.piece_id is None and sl.piece_bend is None for sl in slices)
        s.set_wordpiece(None)
        seen = []
        s.run(tok, raw, 0, seen.append)
        assert all(sl.piece_id is None and sl.n_pieces is None for sl in seen)
