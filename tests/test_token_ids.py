"""Every token looked up in a vocabulary on the device (dtk_batch_set_vocab, dtk_tally of include/datok_gpu.h), GPU tier:
the kernel of dtk_tokenid.hip and its plumbing through batch, pipeline and stream.  Every check is made two ways: the
delivered ids equal the definition of tests/tokenids.py applied to the SAME run's delivered tok_bstart / tok_bend /
tok_off and text, for all documents; and for unflagged documents the keys equal the oracle's surfaces.  The result is
exact: every comparison is an equality."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

import bigsigma
import blocked
import streamcorpus
import tokenids
from test_event_list import _edge_documents, _pipeline_documents
from tokenids import LAST_BYTE, PREFIXES

NO_BYTE_OFFSETS = 512
MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")
MODELS_ENTRIES = ("tokenizer_de.matok:entries", "tokenizer_de.datok:entries")    # the same automata, the stream as 16-bit entries
REPL = b"\xef\xbf\xbd"


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


@contextmanager
def hash_bits(n):
    import datok_amd
    L = datok_amd.lib()
    assert L.dtk_debug_configure(b"VOCAB_HASH_BITS", str(n).encode()) == 0
    try:
        yield
    finally:
        assert L.dtk_debug_configure(b"VOCAB_HASH_BITS", b"-1") == 0


_hip = []


def _runtime():
    """The HIP runtime the library itself is linked against (a lookup on the library's own handle finds it)."""
    if not _hip:
        import datok_amd
        h = C.CDLL(datok_amd.lib()._name)
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        _hip.append(h)
    return _hip[0]


def _from_device(ptr, n, dt):
    out = np.zeros(n, dt)
    if n:
        assert ptr and _runtime().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


class DeviceInput:
    """The text in a device buffer of exactly `total` bytes -- nothing behind its last byte belongs to the caller -- and
    the offsets beside it (dtk_batch_set_input_device)."""

    def __init__(self, text, off):
        h = _runtime()
        self.text, self.off = C.c_void_p(), C.c_void_p()
        off = np.ascontiguousarray(off, dtype=np.uint64)
        assert h.hipMalloc(C.byref(self.text), max(len(text), 1)) == 0 and h.hipMalloc(C.byref(self.off), off.nbytes) == 0
        text = np.ascontiguousarray(text, dtype=np.uint8)
        if len(text):
            assert h.hipMemcpy(self.text, text.ctypes.data, len(text), 1) == 0
        assert h.hipMemcpy(self.off, off.ctypes.data, off.nbytes, 1) == 0

    def close(self):
        for p in (self.text, self.off):
            if p.value:
                assert _runtime().hipFree(p) == 0
                p.value = None


_surfaces = {}


def oracle_surfaces(om, key, docs):
    """Per document the surfaces the oracle's writer prints (TOKENS: one line per token, an empty line per TextEnd), or
    None for a document the oracle flags.  Computed once per key and shared, read only."""
    if key not in _surfaces:
        out = []
        for doc in docs:
            st = om.transduce_doc(doc, 0).status
            out.append(None if st else [l for l in om.transduce(doc, 1)[0].split(b"\n") if l])
        _surfaces[key] = out
    return _surfaces[key]


def _assert_ids(ids, n_unknown, r, text, off, words, surfaces=None):
    """The delivered ids against the definition on the same run's delivered rows; returns (keys, expected ids)."""
    keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)
    exp = tokenids.expected_ids(words, keys)
    assert ids.dtype == np.int32 and ids.shape == exp.shape, (ids.dtype, ids.shape, exp.shape)
    bad = np.flatnonzero(ids != exp)
    assert not len(bad), (len(bad), bad[:4], ids[bad[:4]], exp[bad[:4]], [keys[i] for i in bad[:4]])
    assert n_unknown == int((exp < 0).sum())
    if surfaces is not None:
        n = 0
        for d, s in enumerate(surfaces):
            if s is None or int(r.status[d]):
                continue
            assert keys[int(r.tok_off[d]):int(r.tok_off[d + 1])] == s, d
            n += 1
        assert n > 0
    return keys, exp


def _run(tok, docs, vocab, batch=None, tally=None, ids_home=True, device_input=False, flags=0):
    """(ids, n_unknown, BatchResult, text, doc_off) of one run with the vocabulary attached."""
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
        b.set_vocab(vocab, tally=tally, ids_home=ids_home)
        b.run(tok, flags)
        r = b.result()
        ids, n_unknown = b.token_ids()
        assert len(ids) == b.totals()["n_tokens"]
        return ids, n_unknown, r, text, off
    finally:
        if batch is None:
            b.close()
        if dev is not None:
            dev.close()


# ----------------------------------------------------------------------------------------- 1: shipped models
@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS_DE)
def test_shipped_models(gpu, oracle_models, model):
    """Long running text, three texts in one document, 71 tokens of 1000 bytes, and the edge documents (every length of
    two texts, runs of empty documents).  The vocabulary is every second distinct oracle surface in sorted order, so
    known and unknown ids both occur.  The device view, copied back, is the host view."""
    import datok_amd
    docs = blocked.five_documents() + _edge_documents()[::5]
    surfaces = oracle_surfaces(oracle_models(model), model, docs)
    words = sorted({s for doc in surfaces if doc is not None for s in doc})[::2]
    assert len(words) > 300
    vocab = datok_amd.Vocab(words)
    assert vocab.size == len(words)
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    with _B()(len(text), len(docs)) as b:
        ids, n_unknown, r, text, off = _run(gpu(model), docs, vocab, batch=b)
        keys, exp = _assert_ids(ids, n_unknown, r, text, off, words, surfaces)
        assert (ids >= 0).any() and (ids < 0).any() and 0 < n_unknown < len(ids)
        assert int(ids.max()) < len(words) and len(ids) > 50000
        v = b.token_ids(device=True)
        assert int(v.n_tok) == len(ids) and int(v.n_unknown) == n_unknown
        assert np.array_equal(_from_device(v.tok_id, len(ids), np.int32), ids)
        again, n2 = b.token_ids(copy=False)                       # a second call hands out the same block
        assert np.array_equal(again, ids) and n2 == n_unknown


# ----------------------------------------------------------------------------------- 2: wave and block edges
def _letter_docs(n_tok):
    """n_tok tokens of one letter each in documents with empty ones first, last and in runs in the middle: the first
    token begins at byte 0 of the text and the last one ends at its last byte."""
    letters = [bytes([97 + k % 10]) for k in range(n_tok)]
    k = max(n_tok // 3, 1)
    parts = [letters[:k], letters[k:2 * k], letters[2 * k:]]
    docs = [b"", b""]
    for i, p in enumerate(parts):
        if p:
            docs.append(b" ".join(p))
        docs += [b""] * (3 if i < 2 else 2)
    return docs


@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_wave_and_block_edges(gpu, device_input):
    """1, 63, 64, 65, 255, 256 and 257 tokens in a batch (a wave has 64 lanes, a block 256 threads), with equal
    neighbours in tok_off, and a batch without a token; host input and a device buffer of exactly `total` bytes."""
    import datok_amd
    words = [b"a", b"c", b"e", b"g", b"i", b"ab", b""]
    vocab = datok_amd.Vocab(words)
    tok = gpu(MODELS_DE[0])
    with _B()(4096, 16) as b:
        for n_tok in (1, 63, 64, 65, 255, 256, 257):
            docs = _letter_docs(n_tok)
            ids, n_unknown, r, text, off = _run(tok, docs, vocab, batch=b, device_input=device_input)
            assert len(ids) == n_tok and not r.status[np.diff(off.astype(np.int64)) > 0].any(), n_tok
            keys, exp = _assert_ids(ids, n_unknown, r, text, off, words)
            d_of = np.repeat(np.arange(len(docs)), np.diff(r.tok_off.astype(np.int64)))
            assert int(off[d_of[0]]) + int(r.tok_bstart[0]) == 0                        # the first token at byte 0 of the text
            assert int(off[d_of[-1]]) + int(r.tok_bend[-1]) == len(text)                # ... the last one ends at its last byte
            assert (np.diff(r.tok_off.astype(np.int64)) == 0).sum() >= 8
            assert keys == [bytes([97 + k % 10]) for k in range(n_tok)]
        ids, n_unknown, r, text, off = _run(tok, [b"", b"  ", b""], vocab, batch=b, device_input=device_input)
        assert len(ids) == 0 and n_unknown == 0 and ids.dtype == np.int32


# ------------------------------------------------------------------------------- 3: collisions on the device
def _word4(n):
    return ("\U00010330" * n).encode()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [0, 2])
def test_collisions_on_the_device(gpu, bits):
    """With 0 and 2 bits of the hash every word shares one resp. four buckets and one tag: the bytes decide.  Prefixes of
    one another, words that differ in their last byte, a token of 3000 blank-free bytes (750 runes of four bytes) and a
    word of the same length that differs in its last byte."""
    import datok_amd
    long_a, long_b = _word4(750), _word4(749) + "\U00010331".encode()
    assert len(long_a) == len(long_b) == 3000 and long_a[:-1] == long_b[:-1] and long_a[-1] != long_b[-1]
    words = PREFIXES + LAST_BYTE + [long_b, long_a, b"", b"der"] + tokenids.numbered(40)
    docs = [b" ".join(PREFIXES + [b"abcdef", b"abcdefg", b"b"]), b" ".join(LAST_BYTE + [b"Wortq", b"Wort"]),
            b"der " + long_a + b" die " + long_b + b" " + _word4(749) + b" w7 w39 w40", b""]
    with hash_bits(bits):
        vocab = datok_amd.Vocab(words)
    ids, n_unknown, r, text, off = _run(gpu(MODELS_DE[0]), docs, vocab)
    assert not r.status[:3].any()                                 # (the empty document has DTK_ST_EMPTY_TEXT)
    keys, exp = _assert_ids(ids, n_unknown, r, text, off, words)
    assert long_a in keys and long_b in keys
    assert int(ids[keys.index(long_a)]) == words.index(long_a) and int(ids[keys.index(long_b)]) == words.index(long_b)
    assert int(ids[keys.index(_word4(749))]) == -1 and int(ids[keys.index(b"abcdefg")]) == -1
    assert [int(ids[keys.index(w)]) for w in PREFIXES] == list(range(len(PREFIXES)))
    # the same table built with the whole hash gives the same ids
    ids2, n2, _, _, _ = _run(gpu(MODELS_DE[0]), docs, datok_amd.Vocab(words))
    assert np.array_equal(ids, ids2) and n2 == n_unknown


# -------------------------------------------------------------------------------------------- 4: invalid UTF-8
@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS_DE + MODELS_ENTRIES)
def test_invalid_utf8(gpu, model):
    """A lone 0xFF, a truncated E2 82 and a literal U+FFFD inside tokens.  The vocabulary holds the keys (every invalid
    byte as EF BF BD) and the raw bytes of the same tokens: only the replaced forms match, the truncated sequence gives
    two replacements, and the literal U+FFFD and the invalid byte share an id.  The same batch then runs valid text."""
    import datok_amd
    from datok_amd import corpus
    docs = [b"ab\xffcd ef", b"Preis\xe2\x82 hier und \xe2\x82", "ab\ufffdcd gut".encode(), b"\xff", b"ganz normal", b"",
            b"x\xc3 y\xf0\x9f\x98 z\x80"]
    tok = gpu(model)
    text, off = corpus.concat_docs(docs)
    raw_text = bytes(text)
    with _B()(4096, 8) as b:
        b.set_input(text, off)
        b.run(tok, 0)
        r = b.result()
        keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)
        d_of = np.repeat(np.arange(len(docs)), np.diff(r.tok_off.astype(np.int64)))
        raws = [raw_text[int(off[d]) + int(s):int(off[d]) + int(e)] for d, s, e in zip(d_of, r.tok_bstart, r.tok_bend)]
        changed = [(k, w) for k, w in zip(keys, raws) if k != w]
        assert len(changed) >= 5 and any(REPL + REPL in k for k, _ in changed)
        assert all(len(k) == len(w) + 2 * k.count(REPL) - 2 * w.count(REPL) for k, w in changed)
        words = [w for _, w in changed] + sorted(set(keys)) + [b"\xff", b"\xe2\x82"]
        vocab = datok_amd.Vocab(words)
        ids, n_unknown, r, text, off = _run(tok, docs, vocab, batch=b)
        keys2, exp = _assert_ids(ids, n_unknown, r, text, off, words)
        assert keys2 == keys and n_unknown == 0
        n_raw = len(changed)
        assert (ids >= n_raw).all()                                # no raw form matched
        same = [int(ids[i]) for i, k in enumerate(keys) if k == b"ab" + REPL + b"cd"]
        assert len(same) == 2 and same[0] == same[1]               # the invalid byte and the literal U+FFFD
        # valid text on the same batch object: the fast path, and no trace of the run before
        valid = [b"ganz normal und gut", b"ab cd ef hier Zebra"]
        ids, n_unknown, r, text, off = _run(tok, valid, vocab, batch=b)
        keys, exp = _assert_ids(ids, n_unknown, r, text, off, words)
        assert (ids >= 0).sum() >= 4 and n_unknown >= 1


@pytest.mark.gpu
def test_invalid_utf8_beside_the_letters_of_an_enlarged_model(gpu):
    """bigsigma.enlarged_de(64), whose stream holds 16-bit entries by itself: its new letters on both sides of an \\xff, in
    front of \\xd0 (their lead byte, left alone) and between two \\xff, and a literal U+FFFD.  The vocabulary holds the
    replaced and the raw form of every such token: only the replaced forms match."""
    import datok_amd
    from datok_amd import corpus
    docs = bigsigma.invalid_documents()
    om = bigsigma.oracle_of(bigsigma.enlarged_de(64))
    tok = gpu("de64.matok")
    text, off = corpus.concat_docs(docs)
    raw_text = bytes(text)
    l = [x.encode() for x in bigsigma.LETTERS[:5]]
    with _B()(4096, 8) as b:
        b.set_input(text, off)
        b.run(tok, 0)
        r = b.result()
        keys = tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)
        d_of = np.repeat(np.arange(len(docs)), np.diff(r.tok_off.astype(np.int64)))
        raws = [raw_text[int(off[d]) + int(s):int(off[d]) + int(e)] for d, s, e in zip(d_of, r.tok_bstart, r.tok_bend)]
        changed = [(k, w) for k, w in zip(keys, raws) if k != w]
        for want in (l[0] + l[1] + REPL + l[2] + l[3], b"Preis" + l[0] + REPL, l[1] + REPL, REPL + l[2] + REPL, l[4] + 3 * REPL,
                     b"z" + REPL + l[4]):
            assert want in [k for k, _ in changed], want
        words = [w for _, w in changed] + sorted(set(keys)) + [b"\xff", b"\xd0", l[1] + b"\xd0"]
        vocab = datok_amd.Vocab(words)
        ids, n_unknown, r, text, off = _run(tok, docs, vocab, batch=b)
        surfaces = oracle_surfaces(om, "de64 invalid", docs)
        keys2, exp = _assert_ids(ids, n_unknown, r, text, off, words, surfaces)
        assert keys2 == keys and n_unknown == 0
        assert (ids >= len(changed)).all()                         # no raw form matched
        same = [int(ids[i]) for i, k in enumerate(keys) if k == l[0] + l[1] + REPL + l[2] + l[3]]
        assert len(same) == 2 and same[0] == same[1]               # the invalid byte and the literal U+FFFD


# --------------------------------------------------------------------------------------------------- 5: tally
@pytest.mark.gpu
def test_tally(gpu):
    """read() is the bincount of the expected ids with the unknown tokens in the last slot; counts accumulate over two
    runs; a second token_ids() call, result() and download_begin() on the same run add nothing; reset() zeroes."""
    import datok_amd
    tok = gpu(MODELS_DE[0])
    docs = _pipeline_documents()[:12] + [b"", b"der die das der"]
    words = [b"der", b",", b".", b"die", b"und", b"nicht da", b"das"] + tokenids.numbered(3000) + [b"in", b"zu"]
    vocab = datok_amd.Vocab(words)
    tally = datok_amd.Tally(vocab)
    assert tally.read().dtype == np.uint64 and len(tally.read()) == len(words) + 1 and not tally.read().any()
    with _B()(1 << 16, 16) as b:
        ids, n_unknown, r, text, off = _run(tok, docs, vocab, batch=b, tally=tally)
        _, exp = _assert_ids(ids, n_unknown, r, text, off, words)
        one = tokenids.expected_counts(words, exp)
        assert int(one[-1]) == n_unknown > 0 and one[:5].all() and int(one[len(words) - 2]) > 0
        assert np.array_equal(tally.read(), one)
        b.token_ids(); b.token_ids(device=True); b.download_begin(); b.result()
        assert np.array_equal(tally.read(), one)
        ids2, _, _, _, _ = _run(tok, docs, vocab, batch=b, tally=tally, ids_home=False)     # a second run adds again
        assert np.array_equal(ids2, ids) and np.array_equal(tally.read(), 2 * one)
        tally.reset()
        assert not tally.read().any()
        b.token_ids()
        assert not tally.read().any()                              # ... and the finished run is not added again


@pytest.mark.gpu
@pytest.mark.parametrize("hot_at", ["first", "last"])
def test_tally_contention(gpu, hot_at):
    """"der " 5000 times: every lane of every wave adds to one counter -- the one of index 0, counted in the block's LDS
    first, and the one of the last index of a 5000-word vocabulary, which goes straight to memory."""
    import datok_amd
    words = tokenids.numbered(4999)
    words = [b"der"] + words if hot_at == "first" else words + [b"der"]
    vocab = datok_amd.Vocab(words)
    tally = datok_amd.Tally(vocab)
    ids, n_unknown, r, text, off = _run(gpu(MODELS_DE[0]), [b"der " * 5000, b"w1 w4998 x"], vocab, tally=tally)
    _, exp = _assert_ids(ids, n_unknown, r, text, off, words)
    counts = tally.read()
    assert np.array_equal(counts, tokenids.expected_counts(words, exp))
    assert int(counts[words.index(b"der")]) == 5000 and int(counts[-1]) == 1 and int(counts.sum()) == 5003


# ------------------------------------------------------------------------------------------------ 6: pipeline
@pytest.mark.gpu
@pytest.mark.parametrize("fields", [True, False])
def test_pipeline(gpu, fields):
    """64 documents of 2-6 KB in slices of 32 KB, depth 3: the slices' ids joined are the ids of the same documents as
    one batch, and the tally is their bincount -- with result fields on the pipeline (the ids come home with the slice)
    and without them (a tally alone: the ids are read on demand)."""
    import datok_amd
    from datok_amd import corpus
    B = _B()
    tok = gpu(MODELS_DE[0])
    docs = _pipeline_documents()
    surfaces = sorted({w for d in docs for w in d.split()})
    words = surfaces[::3] + [b",", b".", b"der"]
    vocab = datok_amd.Vocab(words)
    ids1, n_unknown1, r, text, off = _run(tok, docs, vocab)
    _, exp = _assert_ids(ids1, n_unknown1, r, text, off, words)
    assert 0 < n_unknown1 < len(ids1)
    tally = datok_amd.Tally(vocab)
    got, unknown = [], []

    def on_slice(first, n, b):
        ids, n_unknown = b.token_ids()
        assert len(ids) == b.totals()["n_tokens"]
        got.append(ids)
        unknown.append(n_unknown)
    with datok_amd.Pipeline(32 << 10, 64, depth=3) as p:
        p.set_vocab(vocab, tally=tally, ids_home=fields)
        if fields:
            p.set_result_fields(B.R_CSR | B.R_STATUS)
        p.run(tok, text, off, 0, on_slice)
        assert len(got) >= 6
        assert np.array_equal(np.concatenate(got), ids1) and sum(unknown) == n_unknown1
        assert np.array_equal(tally.read(), tokenids.expected_counts(words, exp))
        p.run(tok, text, off, 0, None)                            # counts only: no callback, nothing per token comes home
        assert np.array_equal(tally.read(), 2 * tokenids.expected_counts(words, exp))
        p.run(tok, text, off, NO_BYTE_OFFSETS, None)              # a run without byte offsets has no ids and adds nothing
        assert np.array_equal(tally.read(), 2 * tokenids.expected_counts(words, exp))


# -------------------------------------------------------------------------------------------------- 7: stream
@pytest.mark.gpu
@pytest.mark.parametrize("ids_home", [True, False])
def test_stream(gpu, ids_home):
    """64 KB of German text at Stream(16384), four slices, with a token of 300 bytes across byte S of the first window: the slices'
    tok_id joined are the ids of the same text as one document.  With ids_home=False a tally alone: no slice brings
    ids, and the counts are the stream's."""
    import datok_amd
    tok = gpu(MODELS_DE[0])
    raw = streamcorpus.construct_stream("token300", 0) + b" " + streamcorpus.running_text(24 << 10, seed=11)
    words = sorted({w for w in raw.split()})[::2] + [b",", b".", b"a" * 300]
    vocab = datok_amd.Vocab(words)
    ids1, n_unknown1, r, text, off = _run(tok, [raw], vocab)
    keys, exp = _assert_ids(ids1, n_unknown1, r, text, off, words)
    assert not r.status.any() and b"a" * 300 in keys and 0 < n_unknown1 < len(ids1)
    tally = datok_amd.Tally(vocab)
    slices = []
    with datok_amd.Stream(streamcorpus.S) as s:
        s.set_vocab(vocab, tally=tally, ids_home=ids_home)
        assert s.run(tok, raw, 0, slices.append) == 0
        streamcorpus.check_slices(slices, len(raw))
        assert len(slices) >= 3
        straddles = [i for i in range(len(slices[0].tok_bend))
                     if int(slices[0].tok_bstart[i]) < streamcorpus.S < int(slices[0].tok_bend[i])]
        assert len(straddles) == 1
        assert np.array_equal(tally.read(), tokenids.expected_counts(words, exp))
        assert sum(sl.n_unknown for sl in slices) == n_unknown1
        if ids_home:
            assert all(len(sl.tok_id) == len(sl.tok_bend) and sl.tok_id.dtype == np.int32 for sl in slices)
            assert np.array_equal(np.concatenate([sl.tok_id for sl in slices]), ids1)
            assert int(slices[0].tok_id[straddles[0]]) == words.index(b"a" * 300)
        else:
            assert all(sl.tok_id is None for sl in slices)
        out, st = s.transduce(tok, raw, 3)                        # leaves the vocabulary as set: the tally counts again
        assert st == 0 and np.array_equal(tally.read(), 2 * tokenids.expected_counts(words, exp))
        s.set_vocab(None)
        seen = []
        s.run(tok, raw, 0, seen.append)
        assert all(sl.tok_id is None and sl.n_unknown is None for sl in seen)
        assert np.array_equal(tally.read(), 2 * tokenids.expected_counts(words, exp))


# -------------------------------------------------------------------------------------------------- 8: errors
@pytest.mark.gpu
def test_errors(gpu):
    import datok_amd
    from datok_amd import _lib, corpus
    B = _B()
    tok = gpu(MODELS_DE[0])
    vocab, other = datok_amd.Vocab([b"a", b"b"]), datok_amd.Vocab([b"a", b"b", b"c"])

    def code(fn, *a, **kw):
        with pytest.raises(_lib.DatokGpuError) as e:
            fn(*a, **kw)
        return e.value.code
    text, off = corpus.concat_docs([b"a b c", b"", b"b"])
    with B(1024, 4) as b:
        for device in (False, True):
            assert code(b.token_ids, device=device) == _lib.E_STATE            # before a run, without a vocabulary
        b.set_vocab(vocab)
        assert code(b.token_ids) == _lib.E_STATE                               # before a run
        b.set_input(text, off)
        b.run(tok, 0)
        assert b.token_ids()[0].tolist() == [0, 1, -1, 1] and b.token_ids()[1] == 1
        b.set_vocab(None)
        assert code(b.token_ids) == _lib.E_STATE                               # without a vocabulary
        b.set_vocab(vocab)
        b.run(tok, NO_BYTE_OFFSETS)
        for device in (False, True):
            assert code(b.token_ids, device=device) == _lib.E_STATE            # the keys are cut out with the byte offsets
        assert len(b.result().tok_rstart) == 4                                 # (the other results come as before)
        b.run(tok, 0)
        assert b.token_ids()[0].tolist() == [0, 1, -1, 1]
        assert code(b.set_vocab, vocab, tally=datok_amd.Tally(other)) == _lib.E_ARG     # a tally of another vocabulary
        assert datok_amd.lib().dtk_batch_set_vocab(b._h, None, datok_amd.Tally(vocab)._h, 1) == _lib.E_ARG
        assert code(b.set_result_fields, B.R_ALL | 4096) == _lib.E_ARG         # the ids are no result field: 4096 stays unknown
        assert b.token_ids()[0].tolist() == [0, 1, -1, 1]
    if datok_amd.lib().dtk_device_count() > 1:
        datok_amd.lib().dtk_set_device(1)
        try:
            far = datok_amd.Vocab([b"a"])
        finally:
            datok_amd.lib().dtk_set_device(0)
        with B(1024, 4) as b:
            assert code(b.set_vocab, far) == _lib.E_ARG                        # a vocabulary on another device
            assert datok_amd.lib().dtk_tally_create(far._h, C.byref(C.c_void_p())) == _lib.E_ARG
    with datok_amd.Stream(16384) as s:
        v = _lib.TokenIdView()
        assert datok_amd.lib().dtk_stream_token_ids(s._h, C.byref(v)) == _lib.E_STATE   # outside slice_fn
        assert code(s.set_vocab, vocab, tally=datok_amd.Tally(other)) == _lib.E_ARG
    with datok_amd.Pipeline(32 << 10, 16) as p:
        assert code(p.set_vocab, vocab, tally=datok_amd.Tally(other)) == _lib.E_ARG
        p.set_vocab(vocab)
        p.set_vocab(None)
