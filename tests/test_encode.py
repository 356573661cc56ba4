"""Sentences and documents as fixed-length model input rows on the device (dtk_batch_set_encode of include/datok_gpu.h),
GPU tier: the kernels of dtk_encode.hip and their plumbing through batch and pipeline.  Every case compares the delivered
tables with the definition of tests/encode.py applied to the SAME run's delivered tok_off, sentence table and pieces.
The result is exact: every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest

import bigsigma
import craft
import encode
import wordpiece
from encode import Spec
from test_event_list import _pipeline_documents
from test_sentences import _assert_table, _crafted
from test_token_ids import DeviceInput, _assert_ids, _from_device
from test_wordpiece import _assert_pieces, _corpus_vocab, _memory_type, _runtime

NO_BYTE_OFFSETS = 512
MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")
CLS, SEP, PAD = 101, 102, 0
UNITS = ("sentence", "document")


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


@pytest.fixture(scope="module")
def german():
    """A dozen German documents of a few hundred bytes, a vocabulary that splits a real share of their words, and the
    alphabetic words with their piece counts (what a document of a wanted piece count is put together from)."""
    import datok_amd
    docs = [d[:300 + 40 * k].rsplit(b" ", 1)[0] for k, d in enumerate(_pipeline_documents()[:12])]
    words = _corpus_vocab([w for d in _pipeline_documents() for w in d.split()])
    pool = sorted({w for d in _pipeline_documents()[:24] for w in d.split() if w.decode("utf-8", "replace").isalpha()})
    counts = {w: len(wordpiece.split_key(words, w)[0]) for w in pool}
    return dict(docs=docs, words=words, vocab=datok_amd.Vocab(words), pool=pool, counts=counts,
                filler=next(w for w in pool if counts[w] == 1 and len(w) > 2))


def _B():
    import datok_amd
    return datok_amd.Batch


def _doc_of_pieces(g, c, start=0):
    """One sentence without punctuation whose words make exactly c pieces: words of the pool while they fit, the
    one-piece filler where the next would not."""
    out, total, i = [], 0, start
    while total < c:
        w = g["pool"][i % len(g["pool"])]
        i += 1
        if total + g["counts"][w] > c:
            w = g["filler"]
        out.append(w)
        total += g["counts"][w]
    return b" ".join(out)


def _units(unit, r, sen):
    if unit == "document":
        return encode.units_of_documents(r.tok_off)
    return encode.units_of_sentences(r.tok_off, sen.sen_off, sen.sen_tok_end)


def _device_encoded(b):
    """The device view, copied back: its pointers are device memory -- the kind hipMalloc hands out -- whatever rows_home
    has brought home beside them, and nowhere near the host view's page-locked arrays."""
    import datok_amd
    v, host = b.encoded(device=True), b.encoded(copy=False)
    h = _runtime()
    probe = C.c_void_p()
    assert h.hipMalloc(C.byref(probe), 64) == 0
    try:
        device_kind = _memory_type(probe.value)
    finally:
        assert h.hipFree(probe) == 0
    for name in ("unit_row_off", "input_ids", "row_len", "row_piece0", "word_id"):
        ptr, arr = getattr(v, name), getattr(host, name)
        if name == "word_id" and arr is None:
            assert not ptr
            continue
        assert ptr and _memory_type(ptr) == device_kind, (name, _memory_type(ptr), device_kind)
        if arr.size:
            assert _memory_type(arr.ctypes.data) != device_kind, name
            assert not (arr.ctypes.data <= ptr < arr.ctypes.data + arr.nbytes), name
    nu, nr, ml = int(v.n_units), int(v.n_rows), int(v.max_len)
    return datok_amd.Encoded(_from_device(v.unit_row_off, nu + 1, np.uint64), _from_device(v.input_ids, nr * ml, np.int32).reshape(nr, ml),
                             _from_device(v.row_len, nr, np.uint32), _from_device(v.row_piece0, nr, np.uint64),
                             _from_device(v.word_id, nr * ml, np.int32).reshape(nr, ml) if v.word_id else None,
                             nu, nr, int(v.n_cut), ml)


def _same(a, b):
    return ((a.n_units, a.n_rows, a.n_cut, a.max_len) == (b.n_units, b.n_rows, b.n_cut, b.max_len) and
            all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("unit_row_off", "input_ids", "row_len", "row_piece0")) and
            ((a.word_id is None and b.word_id is None) or np.array_equal(a.word_id, b.word_id)))


def _check(b, spec, unit, what=""):
    """The batch's finished run against the definition; returns (Encoded, BatchResult, Pieces, pieces per unit)."""
    e, r, p = b.encoded(), b.result(), b.pieces()
    units = _units(unit, r, b.sentences() if unit == "sentence" else None)
    encode.assert_equal(e, encode.expected(spec, units, p.piece_off, p.piece_id), what)
    assert _same(_device_encoded(b), e), what
    return e, r, p, [int(p.piece_off[t1]) - int(p.piece_off[t0]) for t0, t1, _ in units]


def _run(tok, docs, vocab, spec, unit, batch=None, rows_home=True, pieces_home=True, device_input=False, first="result"):
    """One run with the split and the encoding attached, checked; `first`: what is asked of the run first."""
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    b = batch or _B()(max(len(text), 1), max(len(docs), 1))
    dev = None
    try:
        if device_input:
            dev = DeviceInput(text, off)
            b.set_input_device(dev.text.value, dev.off.value, len(docs), len(text), keep=dev, doc_off_host=off)
        else:
            b.set_input(text, off)
        b.set_wordpiece(vocab, pieces_home=pieces_home)
        b.set_encode(unit=unit, rows_home=rows_home, **spec.kw())
        b.run(tok, 0)
        if first == "result":
            b.result()
        elif first == "device":
            b.encoded(device=True)
        return _check(b, spec, unit, (unit, spec.kw(), rows_home, pieces_home, device_input, first))
    finally:
        if batch is None:
            b.close()
        if dev is not None:
            dev.close()


# ----------------------------------------------------------------------------- 1: both units, the window edges
@pytest.mark.gpu
@pytest.mark.parametrize("max_len", [5, 64, 65, 128, 513])
@pytest.mark.parametrize("unit", UNITS)
def test_window_edges(gpu, german, unit, max_len):
    """max_len below, at and above a wave's reach and not a multiple of four; stride 0, 1 and body - 1.  Besides running
    text the batch holds one-sentence documents put together word by word for exactly body, body + 1, body + step and
    body + step + 1 pieces, for every stride.  One run per model; each further stride encodes the finished run anew."""
    import datok_amd
    body = max_len - 2
    strides = sorted({0, 1, body - 1})
    edges = {s: (body, body + 1, 2 * body - s, 2 * body - s + 1) for s in strides}
    targets = sorted({c for s in strides for c in edges[s]})
    docs = german["docs"] + [b""] + [_doc_of_pieces(german, c, 7 * k) for k, c in enumerate(targets)]
    for model in MODELS_DE:
        with _B()(1 << 17, 64) as b:
            for k, stride in enumerate(strides):
                spec = Spec(max_len, CLS, SEP, PAD, stride, word_ids=k != 1)
                if k == 0:
                    e, r, p, ns = _run(gpu(model), docs, german["vocab"], spec, unit, batch=b)
                    assert not (r.status & ~np.uint32(datok_amd.ST_EMPTY_TEXT)).any() and (np.diff(p.piece_off.astype(np.int64)) > 1).sum() > 20
                else:
                    b.set_encode(unit=unit, **spec.kw())
                    e, r, p, ns = _check(b, spec, unit, (model, unit, max_len, stride))
                assert all(c in ns for c in edges[stride]), (model, stride, edges[stride], sorted(ns)[-8:])
                assert e.n_cut == sum(n > body for n in ns) > 0 and e.n_rows > e.n_units


# -------------------------------------------------------------------------------------- 2: units without a piece
@pytest.mark.gpu
@pytest.mark.parametrize("unit", UNITS)
def test_empty_and_blank_documents(gpu, german, unit):
    """An empty document and one of blanks only: a unit of no piece under DOCUMENT -- the row of the specials alone --
    and no unit under SENTENCE; then a batch without any token."""
    tok = gpu(MODELS_DE[0])
    spec = Spec(6, CLS, SEP, PAD, 1, word_ids=True)
    with _B()(4096, 8) as b:
        e, r, p, ns = _run(tok, [b"", b"   ", b"Ja. Nein, danke.", b"", b"Gut."], german["vocab"], spec, unit, batch=b)
        if unit == "document":
            assert ns[0] == ns[1] == ns[3] == 0 and e.n_units == 5
            assert e.input_ids[0].tolist() == [CLS, SEP, PAD, PAD, PAD, PAD] and e.row_len[0] == 2
            assert (e.word_id[int(e.unit_row_off[1])] == -1).all()
        else:
            assert e.n_units == 3 and min(ns) > 0
        e, r, p, ns = _run(tok, [b"", b"  ", b""], german["vocab"], spec, unit, batch=b)
        assert (e.n_units, e.n_rows) == ((3, 3) if unit == "document" else (0, 0)) and p.n_pieces == 0
        e, r, p, ns = _run(tok, [b"Und wieder ein Satz."], german["vocab"], Spec(4, -1, -1, 7), unit, batch=b)
        assert e.n_units == 1 and ns[0] >= 5 and e.n_rows == -(-ns[0] // 4) and e.row_len[0] == 4


# ------------------------------------------------------------------------------------------ 3: many scan tiles
@pytest.mark.gpu
def test_seventy_thousand_documents(gpu):
    """70 000 documents of one short word under DOCUMENT with max_len = 4: more than 256 scan tiles of 256 units, so the
    scan of the tile sums takes a second round; sixteen rows share a wave."""
    import datok_amd
    words = [b"[UNK]", b"a", b"##a", b"x"]
    docs = [(b"a", b"aa", b"x", b"", b"aaa a")[k % 5] for k in range(70000)]
    spec = Spec(4, 1, 2, 0, 1, word_ids=True)
    e, r, p, ns = _run(gpu(MODELS_DE[0]), docs, datok_amd.Vocab(words), spec, "document", first="encoded")
    assert e.n_units == 70000 and e.n_rows == 70000 + 2 * 14000 and e.n_cut == 14000 and e.input_ids.nbytes > 1 << 20
    assert e.input_ids[-3:].tolist() == [[1, 1, 2, 2], [1, 2, 2, 2], [1, 2, 1, 2]]


# ------------------------------------------------------------------------- 4: a split that outgrows its block
@pytest.mark.gpu
@pytest.mark.parametrize("unit", UNITS)
def test_split_that_overflows_and_reuse(gpu, german, unit):
    """A vocabulary of single characters and ## characters: every token splits into one piece per rune, the split
    overflows its first block and wrote no piece when the encode first ran.  The delivered rows are complete.  A smaller
    input on the same batch afterwards: no row of the earlier run shows through."""
    import datok_amd
    runes = sorted({c for d in german["docs"] for c in d.decode("utf-8")} - {" ", "\n"})
    words = [b"[UNK]"] + [c.encode() for c in runes] + [b"##" + c.encode() for c in runes]
    vocab = datok_amd.Vocab(words)
    tok = gpu(MODELS_DE[0])
    with _B()(1 << 16, 16) as b:
        e, r, p, ns = _run(tok, german["docs"], vocab, Spec(64, CLS, SEP, PAD, 8, word_ids=True), unit, batch=b)
        n_tok = len(p.piece_off) - 1
        assert p.n_pieces > n_tok + n_tok // 2 + 64 and p.n_unknown == 0           # more than the first block held
        assert e.n_rows > e.n_units
        e, r, p, ns = _run(tok, [b"Ein Satz. Und noch einer.", b"Ja"], vocab, Spec(64, CLS, SEP, PAD, 8, word_ids=True), unit, batch=b)
        assert e.n_rows == e.n_units == (3 if unit == "sentence" else 2)


# ------------------------------------------------------------------------------ 5: where the tables are kept
@pytest.mark.gpu
@pytest.mark.parametrize("pieces_home", [True, False])
@pytest.mark.parametrize("rows_home", [True, False])
def test_homes_and_word_ids(gpu, german, rows_home, pieces_home):
    """rows_home and pieces_home on and off, word_id on and off (NULL when off), whatever is asked of the run first; the
    device view lies in device memory and holds what the host view holds (_check)."""
    tok = gpu(MODELS_DE[1])
    with _B()(1 << 16, 16) as b:
        for k, (unit, word_ids, first) in enumerate([("sentence", True, "result"), ("document", False, "device"),
                                                     ("sentence", False, "encoded"), ("document", True, "result")]):
            spec = Spec(12, CLS, -1 if k == 2 else SEP, PAD, 4, first_window=k == 3, word_ids=word_ids)
            e, r, p, ns = _run(tok, german["docs"][k:], german["vocab"], spec, unit, batch=b, rows_home=rows_home,
                               pieces_home=pieces_home, first=first)
            assert (e.word_id is not None) == word_ids and bool(b.encoded(device=True).word_id) == word_ids
            assert e.n_rows == e.n_units if k == 3 else e.n_rows > e.n_units
            assert _same(b.encoded(copy=False), e)                                 # a second call hands out the same block


# ---------------------------------------------------------------------------------- 6: device-resident input
@pytest.mark.gpu
@pytest.mark.parametrize("unit", UNITS)
def test_device_input_of_exactly_total_bytes(gpu, german, unit):
    """... and the same chain -- walk, split, rows -- where the stream holds 16-bit entries and two documents have bytes
    that do not decode (the encode reads only pieces; the split beneath it reads the stream)."""
    spec = Spec(65, CLS, SEP, PAD, 3, word_ids=True)
    _run(gpu(MODELS_DE[0]), german["docs"], german["vocab"], spec, unit, device_input=True)
    docs = german["docs"] + [b"ab\xffcd ef", b"x\xc3 y\xf0\x9f\x98 z\x80"]
    e, r, p, ns = _run(gpu(MODELS_DE[0] + ":entries"), docs, german["vocab"], spec, unit, device_input=True)
    from datok_amd import corpus
    _assert_pieces(p, r, *corpus.concat_docs(docs), german["words"])
    assert not r.status.any() and len(r.tok_off) == len(docs) + 1 and int(r.tok_off[-1] - r.tok_off[-3]) == 5


# ------------------------------------------------------------------------------------ 7: exact-pass documents
@pytest.mark.gpu
@pytest.mark.parametrize("rows_home", [True, False])
def test_exact_pass_documents_under_sentence(tmp_path, rows_home):
    """The crafted tokenizer of tests/test_sentences.py puts documents into exact_doc: their sentence rows are made on the
    host, and the encode starts only when it is asked for."""
    import datok_amd
    tok, _ = _crafted(tmp_path, "datok", False)
    docs = craft.documents(np.random.default_rng(5), 120)
    words = [b"[UNK]", b"a", b"b", b"##a", b"##b", b".", b"ab"]
    e, r, p, ns = _run(tok, docs, datok_amd.Vocab(words), Spec(6, 1, 2, 0, 2, word_ids=True), "sentence", rows_home=rows_home)
    assert 0 < len(r.exact) < len(docs) and e.n_cut > 0


# ------------------------------------------------------------- 7b: a new input right behind a begun download
@pytest.mark.gpu
def test_new_input_behind_a_begun_download(gpu, german):
    """Ids, pieces, sentence table and rows of one run are enqueued by download_begin() alone, with nothing of them coming
    home, and nobody asks for any of them: the next set_input and run, of other text in documents of the same lengths,
    follow at once.  Only the batch's wait for its derived tables stands between the first run's kernels on the download
    stream and the overwriting of what they read.  The second run's four tables are its own."""
    from datok_amd import corpus
    first = german["docs"][:6]
    other = [d.decode("utf-8", "ignore").encode() for d in (x[:len(f)] for x, f in zip(german["docs"][6:12], first))]
    second = [d + b" " * (len(f) - len(d)) for d, f in zip(other, first)]
    assert [len(d) for d in second] == [len(d) for d in first] and second != first
    spec = Spec(16, CLS, SEP, PAD, 4, word_ids=True)
    tok = gpu(MODELS_DE[0])
    text1, off1 = corpus.concat_docs(first)
    text2, off2 = corpus.concat_docs(second)
    assert np.array_equal(off1, off2)
    with _B()(len(text1), len(first)) as b:
        b.set_vocab(german["vocab"], ids_home=False)
        b.set_wordpiece(german["vocab"], pieces_home=False)
        b.set_encode(unit="sentence", rows_home=False, **spec.kw())
        b.set_input(text1, off1)
        b.run(tok, 0)
        b.download_begin()
        b.set_input(text2, off2)
        b.run(tok, 0)
        e, r, p, ns = _check(b, spec, "sentence", "second run")
        ids, n_unknown = b.token_ids()
        _assert_ids(ids, n_unknown, r, text2, off2, german["words"])
        _assert_pieces(p, r, text2, off2, german["words"])
        _assert_table(b.sentences(), r, off2)
        assert e.n_rows >= e.n_units > len(second) and p.n_pieces > len(ids) > 0


# ----------------------------------------------------------------------------------------------- 8: pipeline
@pytest.mark.gpu
@pytest.mark.parametrize("unit", UNITS)
def test_pipeline(gpu, german, unit):
    """Slices of a few documents: each slice's Encoded is the batch's for the same documents, with unit_row_off and
    row_piece0 from 0.  A vocabulary, a tally and R_SENTENCES beside the spec give what they give without it."""
    import datok_amd
    B = _B()
    tok = gpu(MODELS_DE[0])
    docs = [d[:700].rsplit(b" ", 1)[0] for d in _pipeline_documents()[:24]]
    spec = Spec(48, CLS, SEP, PAD, 5, word_ids=True)
    vocab = german["vocab"]
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    with B(1 << 16, 32) as b:
        e1, r1, p1, _ = _run(tok, docs, vocab, spec, unit, batch=b)
        s1 = b.sentences()
    first_unit = s1.sen_off.astype(np.int64) if unit == "sentence" else np.arange(len(docs) + 1)
    tally = datok_amd.Tally(vocab)
    seen = {}

    def on_slice(first, n, b):
        got = dict(ids=b.token_ids()[0], pieces=b.pieces().piece_id, sen=b.sentences().sen_tok_end)
        if seen["spec"]:
            got["enc"] = b.encoded()
        seen["slices"].append((first, n, got))
    with datok_amd.Pipeline(4 << 10, 4, depth=3) as p:
        p.set_vocab(vocab, tally=tally)
        p.set_wordpiece(vocab)
        p.set_result_fields(B.R_CSR | B.R_STATUS | B.R_SENTENCES)
        runs = {}
        for with_spec in (False, True):
            seen.update(spec=with_spec, slices=[])
            tally.reset()
            if with_spec:
                p.set_encode(unit=unit, **spec.kw())
            p.run(tok, text, off, 0, on_slice)
            runs[with_spec] = (seen["slices"], tally.read())
        p.run(tok, text, off, NO_BYTE_OFFSETS, None)                   # a run without byte offsets has no rows
        p.set_encode(None)
    plain, coded = runs[False], runs[True]
    assert len(coded[0]) >= 5 and np.array_equal(plain[1], coded[1])
    for (f0, n0, g0), (f1, n1, g1) in zip(plain[0], coded[0]):
        assert (f0, n0) == (f1, n1) and all(np.array_equal(g0[k], g1[k]) for k in ("ids", "pieces", "sen"))
    for first, n, got in coded[0]:
        e = got["enc"]
        u0, u1 = int(first_unit[first]), int(first_unit[first + n])
        r0, r1_ = int(e1.unit_row_off[u0]), int(e1.unit_row_off[u1])
        assert e.n_units == u1 - u0 and e.n_rows == r1_ - r0 and int(e.unit_row_off[0]) == 0
        assert np.array_equal(e.unit_row_off.astype(np.int64), e1.unit_row_off[u0:u1 + 1].astype(np.int64) - r0)
        assert np.array_equal(e.input_ids, e1.input_ids[r0:r1_]) and np.array_equal(e.row_len, e1.row_len[r0:r1_])
        assert np.array_equal(e.word_id, e1.word_id[r0:r1_])
        piece0 = int(p1.piece_off[int(r1.tok_off[first])])              # the slice's first piece in the batch
        assert np.array_equal(e.row_piece0.astype(np.int64), e1.row_piece0[r0:r1_].astype(np.int64) - piece0)
    assert sum(g["enc"].n_rows for _, _, g in coded[0]) == e1.n_rows and sum(g["enc"].n_cut for _, _, g in coded[0]) == e1.n_cut


# ------------------------------------------------------------------------------------------------- 9: errors
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
        b.set_wordpiece(vocab)
        b.set_encode(4, 5, 6, 0, unit="document")
        for device in (False, True):
            assert code(b.encoded, device=device) == _lib.E_STATE                 # before a run
        b.set_input(text, off)
        b.run(tok, 0)
        assert b.encoded().input_ids.tolist() == [[5, 1, 1, 6], [5, 2, 0, 6], [5, 6, 0, 0], [5, 1, 2, 6], [5, 2, 6, 0]]
        b.set_encode(None)
        assert code(b.encoded) == _lib.E_STATE                                    # without a spec: the stage is off
        assert b.pieces().piece_id.tolist() == [1, 1, 2, 0, 1, 2, 2]              # (and nothing else is)
        b.set_encode(4, 5, 6, 0, unit="document", first_window=True)
        assert b.encoded().input_ids.tolist() == [[5, 1, 1, 6], [5, 6, 0, 0], [5, 1, 2, 6]]   # the finished run, under the new spec
        b.set_wordpiece(None)
        for device in (False, True):
            assert code(b.encoded, device=device) == _lib.E_STATE                 # without a split
        b.set_wordpiece(vocab, max_runes=2)
        assert b.encoded().input_ids.tolist() == [[5, 1, 1, 6], [5, 6, 0, 0], [5, 0, 6, 0]]   # ... and under the new split
        for bad in (dict(max_len=2), dict(stride=2), dict(max_len=65536), dict(pad_id=-1), dict(cls_id=-2), dict(unit=2)):
            assert code(b.set_encode, **dict(dict(max_len=4, cls_id=5, sep_id=6, pad_id=0), **bad)) == _lib.E_ARG
        assert b.encoded().n_rows == 3                                            # (a rejected spec changes nothing)
        b.run(tok, NO_BYTE_OFFSETS)
        for device in (False, True):
            assert code(b.encoded, device=device) == _lib.E_STATE                 # the pieces need the byte offsets
        assert len(b.result().tok_rstart) == 4                                    # (the other results come as before)
        b.run(tok, 0)
        assert b.encoded().n_rows == 3
        assert datok_amd.lib().dtk_batch_encoded_host(b._h, None) == _lib.E_ARG
    with datok_amd.Pipeline(32 << 10, 16) as p:
        assert code(p.set_encode, 2, 5, 6, 0) == _lib.E_ARG
        p.set_encode(8, 5, 6, 0)
        p.set_encode(None)
