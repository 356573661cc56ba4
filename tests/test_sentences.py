"""A batch's sentences as rows (DTK_R_SENTENCES, dtk_batch_sentences_host / _device of include/datok_gpu.h), GPU tier:
the kernels of dtk_sentences.hip and the download path.  The delivered table equals, entry for entry, the definition of
tests/sentences.py applied to the same run's delivered arrays, and, document by document, the rows that the definition
gives on the oracle's calls."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import craft
import sentences
from conftest import MODELS
from test_event_list import _edge_documents, _pipeline_documents

NEWLINE_AFTER_EOT, OFFSETS_ONLY, NO_BYTE_OFFSETS, NO_RUNE_OFFSETS = 16, 256, 512, 1024
MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")
NAMES = ("sen_off", "sen_tok_end", "sen_bstart", "sen_bend", "sen_rstart", "sen_rend", "text_sen_end")


@pytest.fixture(scope="module")
def gpu():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = datok_amd.load_tokenizer_file(os.path.join(MODELS, name))
            assert cache[name] is not None
        return cache[name]
    return get


def _B():
    import datok_amd
    return datok_amd.Batch


def _fields():
    B = _B()
    return B.R_SENTENCES | B.R_ALL


_hip = []


def _from_device(ptr, n, dt):
    """n elements of a device array, copied back through the HIP runtime the library itself has loaded."""
    if not _hip:
        # (a lookup on the library's own handle searches what it is linked against: a process that has also imported
        #  torch holds a second runtime, which does not know the library's memory)
        import datok_amd
        _hip.append(C.CDLL(datok_amd.lib()._name))
        _hip[0].hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(n, dt)
    if n:
        assert ptr and _hip[0].hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def _expected_oracle(om, doc, flags):
    """(rows of one document by the definition on the oracle's calls, oracle status)."""
    exp = om.transduce_doc(doc, flags)
    firsts, n_tok = sentences.from_calls(om.events(doc)[0])
    if exp.status & 1:
        return None, exp.status
    assert n_tok == len(exp.tok_bend)
    return sentences.rows_of(firsts, n_tok, exp.tok_bstart, exp.tok_bend, exp.tok_rstart, exp.tok_rend, exp.text_tok_end), exp.status


def _assert_table(t, r, off, runes=True):
    """The delivered table against tests/sentences.py on the same run's delivered arrays: entry for entry, dtypes too."""
    e = sentences.from_bitmaps(r.ev_bits, off, r.tok_off, r.tok_bend, r.tok_bstart, r.tok_rstart if runes else None,
                               r.tok_rend if runes else None, r.text_off, r.text_tok_end, r.exact)
    assert t.n_sen == e["n_sen"], (t.n_sen, e["n_sen"])
    for name in NAMES:
        got, exp = getattr(t, name), e[name]
        if exp is None:
            assert got is None, name
            continue
        assert got is not None and got.dtype == exp.dtype and got.shape == exp.shape, (name, got.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (name, np.flatnonzero(got != exp)[:4])
    assert int(t.sen_off[0]) == 0 and int(t.sen_off[-1]) == t.n_sen
    return e


def _assert_oracle(t, r, docs, om, flags=0, runes=True, ids=None):
    """Every document's rows against the definition on the oracle's calls; returns how many were compared."""
    n = 0
    for d in (range(len(docs)) if ids is None else ids):
        exp, _ = _expected_oracle(om, docs[d], flags)
        if exp is None:                                   # (window overflow: the reference dies there)
            continue
        got = t.doc(d)
        for name in ("sen_tok_end", "sen_bstart", "sen_bend") + (("sen_rstart", "sen_rend") if runes else ()):
            assert np.array_equal(got[name], exp[name]), (d, docs[d][:60], name, got[name][:6], exp[name][:6])
        x0, x1 = int(r.text_off[d]), int(r.text_off[d + 1])
        assert np.array_equal(t.text_sen_end[x0:x1], exp["text_sen_end"]), (d, docs[d][:60])
        n += 1
    return n


def _run(tok, docs, fields, flags=0, batch=None, chunking=None, device=True):
    """(host table, BatchResult, doc_off, totals) of one run; the device view, copied back, equals the host view."""
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    b = batch or _B()(max(len(text), 1), len(docs))
    try:
        if chunking is not None:
            b.set_chunking(*chunking[:2], extend=chunking[2])
        b.set_input(text, off)
        b.set_result_fields(fields)
        b.run(tok, flags)
        r, tot = b.result(), b.totals()
        t = b.sentences()
        assert t.n_sen <= tot["n_sent"]
        if device:
            v = b.sentences(device=True)
            assert v.n_sen == t.n_sen and v.sen_off
            shape = dict(sen_off=(len(docs) + 1, np.uint64), sen_tok_end=(t.n_sen, np.uint32), sen_bstart=(t.n_sen, np.uint32),
                         sen_bend=(t.n_sen, np.uint32), sen_rstart=(t.n_sen, np.int32), sen_rend=(t.n_sen, np.int32),
                         text_sen_end=(tot["n_texts"], np.uint32))
            for name in NAMES:
                if getattr(t, name) is None:
                    assert getattr(v, name) is None, name
                else:
                    assert np.array_equal(_from_device(getattr(v, name), *shape[name]), getattr(t, name)), name
        return t, r, off, tot
    finally:
        if batch is None:
            b.close()


# ------------------------------------------------------------------------------------------------- 1: edges
@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, NEWLINE_AFTER_EOT])
@pytest.mark.parametrize("model", MODELS_DE)
def test_edges(gpu, oracle_models, model, flags):
    """About 400 documents: every length 0..160 of two texts, runs of empty documents at the head, in the middle and at
    the end of the batch, "a", a lone EOT, texts that end in an EOT."""
    docs = _edge_documents()
    t, r, off, tot = _run(gpu(model), docs, _fields(), flags)
    _assert_table(t, r, off)
    assert _assert_oracle(t, r, docs, oracle_models(model), flags) == len(docs)
    per_doc = np.diff(t.sen_off.astype(np.int64))
    assert int(t.sen_off[0]) == 0 and int(t.sen_off[-1]) == t.n_sen <= tot["n_sent"] and t.n_sen > 1500
    assert per_doc[docs.index(b"a")] == 1 and per_doc[docs.index(b"\x04")] == 0 and per_doc[docs.index(b"   ")] == 0
    assert (per_doc[:9] == 0).all() and (per_doc[-21:] == 0).all() and per_doc.max() > 10
    # every token belongs to exactly one sentence: a document's last row ends at its token count
    last = t.sen_off[1:][per_doc > 0].astype(np.int64) - 1
    assert np.array_equal(t.sen_tok_end[last], np.diff(r.tok_off.astype(np.int64))[per_doc > 0])
    assert (np.diff(r.tok_off.astype(np.int64))[per_doc == 0] == 0).all()


# ------------------------------------------------------------------------- 2: word, thread and tile edges
def _sweep(tok, om, centre, span=200):
    """One pad document of centre - span/2 .. centre + span/2 bytes ("ab ab ab ...": tokens and no boundary, so one row)
    in front of "Ja. Nein! Doch? " repeated: returns, per pad length, the global bits of the second document's
    sentence-first END bits and of the boundaries (SEPS) in front of them."""
    from datok_amd import corpus
    B = _B()
    body = b"Ja. Nein! Doch? " * 24
    exp, _ = _expected_oracle(om, body, 0)
    filler = b"ab " * ((centre + span) // 3 + 1)
    out = []
    with B(centre + span + len(body) + 64, 2) as b:
        b.set_result_fields(B.R_SENTENCES | B.R_TOK_BYTE | B.R_CSR | B.R_STATUS)
        for pad in range(centre - span // 2, centre + span // 2):
            docs = [filler[:pad], body]
            text, off = corpus.concat_docs(docs)
            b.set_input(text, off)
            b.run(tok, 0)
            t, r = b.sentences(), b.result()
            assert not r.status.any() and t.n_sen == 1 + len(exp["sen_tok_end"]) == 73 and t.sen_off.tolist() == [0, 1, 73], pad
            assert int(t.sen_tok_end[0]) == int(r.tok_off[1]) and int(t.sen_bstart[0]) == 0, pad
            for name in ("sen_tok_end", "sen_bstart", "sen_bend", "sen_rstart", "sen_rend"):
                assert np.array_equal(getattr(t, name)[1:], exp[name]), (pad, name)
            first_tok = np.concatenate([[0], t.sen_tok_end[1:-1]]).astype(np.int64)
            bit0 = pad + 1                                           # bit of cursor 0 of the second document
            first_bits = bit0 + r.tok_bend[int(r.tok_off[1]) + first_tok].astype(np.int64)
            bound_bits = bit0 + t.sen_bend[1:-1].astype(np.int64)    # the SentenceEnd behind a sentence's last token
            out.append((first_bits[1:], bound_bits))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("edge", ["word", "thread", "tile", "two_tiles"])
def test_word_thread_and_tile_edges(gpu, oracle_models, edge):
    """A sentence-first END bit and the boundary in front of it on both sides of a word's, a thread's span's, a tile's
    and the second tile's edge: 200 consecutive pad lengths around each."""
    import datok_amd
    T = datok_amd.lib().dtk_sentences_tile_bits()
    assert T % 32 == 0 and T >= 4096
    unit, centre = {"word": (32, 4000), "thread": (128, 4096), "tile": (T, T), "two_tiles": (T, 2 * T)}[edge]
    model = MODELS_DE[0]
    seen = set()
    for first_bits, bound_bits in _sweep(gpu(model), oracle_models(model), centre):
        for f, s in zip(first_bits.tolist(), bound_bits.tolist()):
            assert s < f
            # the boundary in the unit in front of the END bit's, or both in one: at the unit's last bit / first bit
            if f // unit == s // unit + 1:
                seen.add("split")
            if f % unit == 0:
                seen.add("first at bit 0")
            if s % unit == unit - 1:
                seen.add("boundary at the last bit")
            if f % unit == unit - 1:
                seen.add("first at the last bit")
            if edge in ("tile", "two_tiles") and f // unit == s // unit + 1 and f // T == centre // T:
                seen.add("across the aimed edge")
    want = {"split", "first at bit 0", "boundary at the last bit", "first at the last bit"}
    if edge in ("tile", "two_tiles"):
        want.add("across the aimed edge")
    assert seen >= want, want - seen


# ------------------------------------------------- 3: event-free tiles and the reset at a document start
@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS_DE)
def test_event_free_tiles_and_document_start(gpu, oracle_models, model):
    """A document that overflows the window and leaves whole tiles without an event, an empty document, blanks, a
    normal text: the document behind the overflowed one opens with a sentence of its own."""
    import datok_amd
    T = datok_amd.lib().dtk_sentences_tile_bits()
    docs = [b"Ja. " + b" " * (2 * T + 5000) + b"Nein.", b"", b"   ", b"Gut. Und dann? Ja!", b"Nein."]
    om = oracle_models(model)
    t, r, off, tot = _run(gpu(model), docs, _fields())
    _assert_table(t, r, off)
    assert int(r.status[0]) & 1 and not (r.status[1:] & 1).any()      # (the token-free ones have DTK_ST_EMPTY_TEXT)
    left_out = [d for d in range(len(docs)) if om.transduce_doc(docs[d], 0).status & 1]
    assert left_out == [0]
    assert _assert_oracle(t, r, docs, om) == len(docs) - 1
    per_doc = np.diff(t.sen_off.astype(np.int64)).tolist()
    assert per_doc[1:] == [0, 0, 3, 1] and int(t.sen_bstart[int(t.sen_off[3])]) == 0


# --------------------------------------------------------- 4: after repairs and on every walk shape
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["chunk0", "chunk16", "chunk128", "mispredict", "offsets_only", "no_runes"])
def test_walk_shapes(gpu, oracle_models, shape):
    """The edge documents again: one lane per document, chunk lanes of 16 and 128 bytes, chunks without warm-up (the
    table is read off the bitmaps behind the repair rounds), and the offsets-only flags."""
    chunking = {"chunk0": (0, 8, None), "chunk16": (16, 8, None), "chunk128": (128, 8, None), "mispredict": (16, 0, 0)}.get(shape)
    flags = {"offsets_only": OFFSETS_ONLY, "no_runes": NO_RUNE_OFFSETS}.get(shape, 0)
    model = MODELS_DE[0]
    docs = _edge_documents()
    t, r, off, tot = _run(gpu(model), docs, _fields(), flags, chunking=chunking)
    runes = shape != "no_runes"
    if shape == "mispredict":
        assert tot["repair_rounds"] > 0
    if not runes:
        assert t.sen_rstart is None and t.sen_rend is None and len(r.tok_rstart) == 0
    _assert_table(t, r, off, runes=runes)
    assert _assert_oracle(t, r, docs, oracle_models(model), 0, runes=runes) == len(docs)


@pytest.mark.gpu
def test_no_byte_offsets_is_a_state_error(gpu):
    """The table is keyed on tok_bend: a run with NO_BYTE_OFFSETS has none, with and without the field selected."""
    from datok_amd import _lib, corpus
    B = _B()
    docs = _edge_documents()[:40]
    text, off = corpus.concat_docs(docs)
    with B(len(text), len(docs)) as b:
        b.set_input(text, off)
        for fields in (B.R_SENTENCES | B.R_ALL, B.R_ALL):
            b.set_result_fields(fields)
            b.run(gpu(MODELS_DE[0]), NO_BYTE_OFFSETS)
            r = b.result()                                   # (the other fields come as before)
            assert len(r.tok_rstart) == b.totals()["n_tokens"] and len(r.tok_bend) == 0
            for device in (False, True):
                with pytest.raises(_lib.DatokGpuError) as e:
                    b.sentences(device=device)
                assert e.value.code == _lib.E_STATE
        b.run(gpu(MODELS_DE[0]), 0)                          # the next run has one again
        assert b.sentences().n_sen > 20


# ----------------------------------------------------------------------------- 5: exact-pass documents
def _crafted(tmp_path, kind, triple):
    import datok_amd
    from oracle import oracle as O
    blob = getattr(craft, kind)(triple)
    path = tmp_path / ("crafted%d.%s" % (triple, kind))
    path.write_bytes(blob)
    return datok_amd.load_tokenizer_file(str(path)), O.Model(raw=gzip.decompress(blob))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,triple,flags", [("datok", False, 0), ("matok", True, 0), ("datok", True, 0),
                                               ("matok", False, NEWLINE_AFTER_EOT), ("datok", False, NEWLINE_AFTER_EOT)])
def test_exact_pass_documents(tmp_path, kind, triple, flags):
    """The crafted tokenizers of tests/craft.py: an EOT consumed twice by a double array, three epsilon SentenceEnds at
    one cursor, the newline token at offset 0 under NEWLINE_AFTER_EOT.  Documents the exact pass walked lie between
    regular ones; every row equals the definition on the oracle's calls."""
    tok, om = _crafted(tmp_path, kind, triple)
    docs = craft.documents(np.random.default_rng(5), 120)
    if flags:
        docs += [b"aba \x04\na aaabb\n \x04b a\n\na  b\n  \nb\x04\n\nab .   a aa", b"b\x04\n\nab", b"a b. a", b"a\x04\n\n\na b\x04\n\nb", b"ab. b"]
    t, r, off, tot = _run(tok, docs, _fields(), flags)
    assert 0 < len(r.exact) < len(docs)
    _assert_table(t, r, off)
    assert _assert_oracle(t, r, docs, om, flags) == len(docs)
    # regular documents behind an exact one: their sen_off is what the rows in front of them add up to
    behind = [d + 1 for d in r.exact if d + 1 < len(docs) and d + 1 not in r.exact]
    assert len(behind) > 3
    per_doc = [len(_expected_oracle(om, doc, flags)[0]["sen_tok_end"]) for doc in docs]
    assert np.array_equal(t.sen_off, np.concatenate([[0], np.cumsum(per_doc)]).astype(np.uint64))


# ------------------------------------------------------------------------------------------ 6: capacity
@pytest.mark.gpu
def test_capacity_and_regrowth(gpu, oracle_models):
    """A batch first used for a few bytes, then for "a. " and "Ja. " repeated: the table's arrays grow with the run.  Then the
    SEN_CAP hook sizes the first build for one row: the kernels leave the table alone and report the count, the host
    grows and launches again, and the table is complete."""
    import datok_amd
    model = MODELS_DE[0]
    tok, om = gpu(model), oracle_models(model)
    # ("a." is an abbreviation to the German tokenizer and ends no sentence: the document stays, the rows come from the others)
    many = [b"a. " * 700, b"", b"Ja. " * 700, b"Nein! " * 300]
    with _B()(8192, 4) as b:
        t, r, off, _ = _run(tok, [b"Ein Baum."], _fields(), batch=b)
        assert t.n_sen == 1
        t, r, off, _ = _run(tok, many, _fields(), batch=b)
        assert t.n_sen > 1000 and np.diff(t.sen_off.astype(np.int64)).tolist()[1:] == [0, 700, 300]
        _assert_table(t, r, off)
        assert _assert_oracle(t, r, many, om) == 4
        assert datok_amd.lib().dtk_debug_configure(b"SEN_CAP", b"1") == 0
        try:
            for fields in (_fields(), _B().R_ALL):               # with the download, and on demand
                t2, r2, off2, _ = _run(tok, many, fields, batch=b)
                for name in NAMES:
                    assert np.array_equal(getattr(t2, name), getattr(t, name)), name
        finally:
            assert datok_amd.lib().dtk_debug_configure(b"SEN_CAP", b"-1") == 0
        t, r, off, _ = _run(tok, [b"Ein Baum. Zwei!"], _fields(), batch=b)     # no stale row of the larger run
        assert t.n_sen == 2 and t.sen_off.tolist() == [0, 2] and t.sen_tok_end.tolist() == [3, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("selected", [True, False])
def test_device_view_first_then_host_view(gpu, oracle_models, selected):
    """The device view first (it brings only the count word home), then the host view of the same run: the host call
    copies the block and waits for it.  The batch's previous run left another, longer table in the page-locked block."""
    from datok_amd import corpus
    B = _B()
    model = MODELS_DE[0]
    tok, om = gpu(model), oracle_models(model)
    before, docs = [b"Nein! Doch? " * 2000, b"Ja. " * 3000], [b"Gut. Und dann? Ja!", b"", b"Ein Baum. " * 1500, b"Nein."]
    with B(40000, 4) as b:
        b.set_result_fields((B.R_SENTENCES if selected else 0) | B.R_ALL)
        text, off = corpus.concat_docs(before)
        b.set_input(text, off)
        b.run(tok, 0)
        assert b.sentences().n_sen == 7000
        text, off = corpus.concat_docs(docs)
        b.set_input(text, off)
        b.run(tok, 0)
        if not selected:
            v = b.sentences(device=True)
            assert v.n_sen == 1504
        else:
            v = None
        t = b.sentences(copy=False)            # (no copy: what the call hands out, as it hands it out)
        snap = {name: getattr(t, name).copy() for name in NAMES}
        if v is None:
            v = b.sentences(device=True)
        r = b.result()
        _assert_table(t, r, off)
        for name in NAMES:
            assert np.array_equal(snap[name], getattr(t, name)), name
        assert t.n_sen == v.n_sen == 1504 and _assert_oracle(t, r, docs, om) == 4


# ------------------------------------------------------------------------------------------ 7: pipeline
@pytest.mark.gpu
@pytest.mark.parametrize("selected", [True, False])
def test_pipeline(gpu, oracle_models, selected):
    """64 documents of 2-6 KB in slices of 32 KB, depth 3: every slice's table equals the oracle's rows, with the field
    set on the pipeline (the table comes home with the slice) and without it (built on demand in the callback)."""
    import datok_amd
    from datok_amd import corpus
    B = _B()
    model = MODELS_DE[0]
    om = oracle_models(model)
    docs = _pipeline_documents()
    text, off = corpus.concat_docs(docs)
    seen = []

    def on_slice(first, n, b):
        r = b.result(copy=False)
        t = b.sentences(copy=False)
        assert len(t.sen_off) == n + 1 and t.n_sen == int(t.sen_off[-1]) > n and len(r.tok_bend) == 0
        assert _assert_oracle(t, r, docs[first:first + n], om) == n
        seen.append(n)
    with datok_amd.Pipeline(32 << 10, 64, depth=3) as p:
        p.set_result_fields((B.R_SENTENCES if selected else 0) | B.R_CSR | B.R_STATUS)
        p.run(gpu(model), text, off, 0, on_slice)
    assert sum(seen) == len(docs) and len(seen) >= 6


# -------------------------------------------------------------------------------------------- 8: errors
@pytest.mark.gpu
def test_errors(gpu):
    import datok_amd
    from datok_amd import _lib
    B = _B()
    with B(1024, 4) as b:
        for device in (False, True):
            with pytest.raises(_lib.DatokGpuError) as e:      # before any run
                b.sentences(device=device)
            assert e.value.code == _lib.E_STATE
        with pytest.raises(_lib.DatokGpuError) as e:          # an unknown bit beside it
            b.set_result_fields(B.R_SENTENCES | 4096)
        assert e.value.code == _lib.E_ARG
        b.set_result_fields(B.R_SENTENCES)                    # the bit alone is fine
    with datok_amd.Stream(16384) as s:
        for fields in (B.R_SENTENCES | B.R_TOK_BYTE, B.R_SENTENCES | B.R_TOK_BYTE | 4096):
            with pytest.raises(_lib.DatokGpuError) as e:
                s.set_result_fields(fields)
            assert e.value.code == _lib.E_ARG
        s.set_result_fields(B.R_TOK_BYTE)
    with datok_amd.Pipeline(32 << 10, 16) as p:
        p.set_result_fields(B.R_SENTENCES | B.R_CSR)
        with pytest.raises(_lib.DatokGpuError) as e:
            p.set_result_fields(B.R_SENTENCES | 4096)
        assert e.value.code == _lib.E_ARG
