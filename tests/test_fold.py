"""Token keys folded on the device (dtk_batch_set_fold of include/datok_gpu.h), GPU tier: the folded instantiations of the
kernels of dtk_tokenid.hip and dtk_wordpiece.hip and their plumbing through batch, pipeline and stream.  The delivered
ids, pieces and counters equal the definition of tests/fold.py applied to the SAME run's delivered tok_bstart / tok_bend /
tok_off and text.  The result is exact: every comparison is an equality."""
import numpy as np
import pytest

import bigsigma
import encode
import fold
import streamcorpus
import tokenids
import wordpiece
from fold import ACUTE, AE, DESERET, DIAERESIS, HAND, HAND_REPL_VANISHES, HANGUL, UE, fold_key
from test_event_list import _pipeline_documents
from test_token_ids import DeviceInput
from wordpiece import REPL

MODEL = "tokenizer_de.matok"


@pytest.fixture(scope="module")
def gpu():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bigsigma.device_model(name)[0]
        return cache[name]
    return get


@pytest.fixture(scope="module")
def folds():
    """The mappings of these tests with their device objects, made once: name -> (mapping, Fold)."""
    import datok_amd
    maps = {"hand": HAND, "hand_repl_vanishes": HAND_REPL_VANISHES, "bert": datok_amd.bert_uncased_mapping(), "empty": {}}
    return {k: (m, datok_amd.Fold(m)) for k, m in maps.items()}


def _B():
    import datok_amd
    return datok_amd.Batch


def _u(s):
    return s.encode("utf-8")


# one token each under tokenizer_de: case, a composed and a decomposed umlaut, sharp s, Hangul, a 4-byte pair, a
# source of two targets, marks alone and behind letters
POOL = [_u(w) for w in (UE + "ber", AE + "RGER", "Stra" + chr(0xDF) + "e", "A" + DIAERESIS + "rger", HANGUL + chr(0xAD6D),
                        DESERET + "x", fold.KA + fold.O, "der", "Der", "Haus" + ACUTE, HANGUL, "a" + ACUTE + "b", ACUTE,
                        "ab" + DESERET, AE * 4, "xyz" + UE, "Mann", "x" + DESERET, "x" + UE, "und", "Und", "UND")]


def _mixed_docs(n_tok, last=None):
    """n_tok tokens of POOL in documents with empty ones first, last and in runs in the middle (the layout of
    test_wordpiece._a_docs); `last`: the last token, which ends at the text's last byte."""
    toks = [POOL[(k * 7 + k // len(POOL)) % len(POOL)] for k in range(n_tok)]
    if last is not None:
        toks[-1] = last
    k = max(n_tok // 3, 1)
    docs = [b"", b""]
    for i, part in enumerate([toks[:k], toks[k:2 * k], toks[2 * k:]]):
        if part:
            docs.append(b" ".join(part))
        docs += [b""] * (3 if i < 2 else 2)
    return docs


def _vocabularies(mapping, keys):
    """(id words, split words) from the folded surfaces of the text: three quarters of them whole for the ids; for the
    split a third whole, of the others the first one or two runes as a first piece and the rest behind the prefix."""
    surfaces = sorted({fold_key(mapping, k).decode("utf-8") for k in keys if k} - {""})
    id_words = [_u(s) for k, s in enumerate(surfaces) if k % 4]
    heads, conts, whole = set(), set(), []
    for k, s in enumerate(surfaces):
        n = k % 3
        if n == 0 or len(s) <= n:
            whole.append(_u(s))
        else:
            heads.add(_u(s[:n]))
            conts.add(_u("##" + s[n:]))
    return id_words, [b"[UNK]", b"", b"##"] + whole + sorted(heads - set(whole)) + sorted(conts)


def _keys(r, text, off):
    return tokenids.keys_of_batch(text, off, r.tok_off, r.tok_bstart, r.tok_bend)


def _assert_folded(b, mapping, id_words, wp_words, text, off, max_runes=0):
    """The batch's finished run against the definition under `mapping` (None: no fold); returns (ids, Pieces, keys)."""
    r = b.result()
    keys = _keys(r, text, off)
    ids, n_unknown = b.token_ids()
    p = b.pieces()
    if mapping is None:
        e_ids = tokenids.expected_ids(id_words, keys)
        e_off, e_id, e_bend, e_unknown = wordpiece.expected_pieces(wp_words, text, off, r.tok_off, r.tok_bstart, r.tok_bend,
                                                                   max_runes=max_runes)
    else:
        e_ids = fold.expected_ids(id_words, mapping, keys)
        e_off, e_id, e_bend, e_unknown = fold.expected_pieces(wp_words, mapping, text, off, r.tok_off, r.tok_bstart, r.tok_bend,
                                                              max_runes=max_runes)
    bad = np.flatnonzero(ids != e_ids) if ids.shape == e_ids.shape else None
    assert bad is not None and not len(bad), (bad[:4], ids[bad[:4]], e_ids[bad[:4]], [keys[i] for i in bad[:4]])
    assert n_unknown == int((e_ids < 0).sum())
    assert np.array_equal(p.piece_off, e_off), (p.piece_off[:8], e_off[:8], len(p.piece_off), len(e_off))
    bad = np.flatnonzero(p.piece_id != e_id) if p.piece_id.shape == e_id.shape else None
    assert bad is not None and not len(bad), (bad[:4], p.piece_id[bad[:4]], e_id[bad[:4]])
    bad = np.flatnonzero(p.piece_bend != e_bend)
    assert not len(bad), (bad[:4], p.piece_bend[bad[:4]], e_bend[bad[:4]])
    assert p.n_pieces == len(e_id) and p.n_unknown == e_unknown
    return ids, p, keys


def _run(b, tok, docs, fold_obj, id_vocab, wp_vocab, device_input=False, max_runes=0, tally=None):
    """One run with the vocabulary, the split and the fold attached; returns (text, off, the device buffers to close)."""
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    dev = None
    if device_input:
        dev = DeviceInput(text, off)
        b.set_input_device(dev.text.value, dev.off.value, len(docs), len(text), keep=dev, doc_off_host=off)
    else:
        b.set_input(text, off)
    b.set_vocab(id_vocab, tally=tally)
    b.set_wordpiece(wp_vocab, max_runes=max_runes)
    b.set_fold(fold_obj)
    b.run(tok, 0)
    return text, off, dev


# ------------------------------------------------------------------------- 1: ids and pieces at wave and tile edges
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hand", "bert"])
def test_mixed_text_at_wave_and_tile_edges(gpu, folds, which):
    """Batches of exactly 63 / 64 / 65 / 257 tokens of mixed German text under the hand-written mapping and under
    bert_uncased_mapping(), over vocabularies made of the text's folded surfaces: more than half of the tokens get an id,
    and tokens split behind a rune the fold changed."""
    import datok_amd
    tok = gpu(MODEL)
    mapping, f = folds[which]
    id_words, wp_words = _vocabularies(mapping, [k for k in POOL])
    id_vocab, wp_vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(wp_words)
    with _B()(8192, 16) as b:
        for n_tok in (63, 64, 65, 257):
            text, off, _ = _run(b, tok, _mixed_docs(n_tok), f, id_vocab, wp_vocab)
            ids, p, keys = _assert_folded(b, mapping, id_words, wp_words, text, off)
            assert len(ids) == n_tok and keys[0] == POOL[0]
            assert 2 * int((ids >= 0).sum()) > n_tok                    # (not all unknown)
            behind_folded = 0
            for i, key in enumerate(keys):
                a, z = int(p.piece_off[i]), int(p.piece_off[i + 1])
                if z - a < 2:
                    continue
                bs = int(b.result().tok_bstart[i])
                for q in range(a, z - 1):                               # a cut inside the token: the rune in front of it
                    head = key[:int(p.piece_bend[q]) - bs].decode("utf-8")
                    behind_folded += ord(head[-1]) in mapping
            assert behind_folded > 0, n_tok
            counts = np.diff(p.piece_off.astype(np.int64))
            assert counts.min() == 1 and counts.max() >= 2 and 0 < p.n_unknown < n_tok


# ------------------------------------------------------------------ 2: the buffer's last byte inside a folded rune
@pytest.mark.gpu
@pytest.mark.parametrize("device_input", [False, True])
def test_the_last_byte_is_the_tail_of_a_folded_rune(gpu, folds, device_input):
    """Total lengths of 4k + 1 .. 4k + 4 bytes whose last byte is the second byte of a two-byte rune the fold changes, and
    the fourth of a four-byte one: the results are right, from host input and from a device buffer of exactly that many
    bytes.  (The aligned-read rule, positively: the words read are the buffer's.)"""
    import datok_amd
    tok = gpu(MODEL)
    mapping, f = folds["hand"]
    id_words = [b"xu", _u("x" + fold.deseret), b"f", b"ff", b"fff", b"ffff"]
    words = [b"[UNK]", b"x", b"##u", _u("##" + fold.deseret), b"f", b"##f"]
    id_vocab, vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(words)
    with _B()(4096, 4) as b:
        for last in (_u("x" + UE), _u("x" + DESERET)):
            seen = set()
            for pad in range(4):
                docs = [b"", b"f" * (1 + pad) + b" " + last]
                text, off, dev = _run(b, tok, docs, f, id_vocab, vocab, device_input=device_input)
                try:
                    seen.add(len(text) % 4)
                    ids, p, keys = _assert_folded(b, mapping, id_words, words, text, off)
                    assert keys == [b"f" * (1 + pad), last] and int(p.piece_bend[-1]) == int(b.result().tok_bend[-1]) == len(text)
                    assert bytes(text[-len(last):]) == last
                    assert p.piece_id[-2:].tolist() == ([1, 2] if last[1] == 0xC3 else [1, 3])
                    assert ids.tolist() == [2 + pad, 0 if last[1] == 0xC3 else 1]
                finally:
                    if dev is not None:
                        dev.close()
            assert seen == {0, 1, 2, 3}


# -------------------------------------------------------------------------------- 3: invalid bytes under the fold
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["hand", "hand_repl_vanishes"])
@pytest.mark.parametrize("model", [MODEL, MODEL + ":entries"])
def test_invalid_bytes_under_the_fold(gpu, folds, model, which):
    """A lone 0xD0, a truncated sequence and 0xFF as the text's last byte: each is U+FFFD under the fold -- listed as
    folding to nothing, or unlisted -- and one source byte in piece_bend.  The same batch then runs valid text."""
    import datok_amd
    tok = gpu(model)
    mapping, f = folds[which]
    docs = [b"AB\xffcd ef", b"Preis\xd0 hier", _u(UE) + b"ber\xd0", b"ganz Normal", b"", b"x\xc3 y\xf0\x9f\x98 z\x80",
            _u("A" + DIAERESIS) + b"\xffrger", b"Ende X\xff"]
    words = [b"[UNK]", b"ab", b"##cd", b"abcd", b"##" + REPL, b"##" + REPL + b"cd", b"preis", b"uber", b"x", b"y", b"z", b"ef",
             b"hier", b"ganz", b"normal", b"arger", b"a", b"##rger", b"ende", b"##" + REPL + REPL + REPL, b"Preis", b"##\xd0", b"##\xff"]
    vocab = datok_amd.Vocab(words)
    with _B()(4096, 8) as b:
        text, off, _ = _run(b, tok, docs, f, vocab, vocab)
        ids, p, keys = _assert_folded(b, mapping, words, words, text, off)
        r = b.result()
        i = keys.index(b"AB" + REPL + b"cd")
        got = (p.piece_id[int(p.piece_off[i]):int(p.piece_off[i + 1])].tolist(), p.piece_bend[int(p.piece_off[i]):int(p.piece_off[i + 1])].tolist())
        if which == "hand":
            assert got == ([1, 5], [2, 5]) and int(ids[i]) == -1
        else:
            assert got == ([3], [5]) and int(ids[i]) == 3               # the replaced byte vanished: abcd
        assert bytes(text[-1:]) == b"\xff" and int(p.piece_bend[-1]) == int(r.tok_bend[-1])
        assert (p.piece_id < 20).all() and (ids < 20).all()             # no raw and no unfolded form matched
        text, off, _ = _run(b, tok, [b"Ganz normal", b"AB cd Ef HIER x"], f, vocab, vocab)
        ids, p, keys = _assert_folded(b, mapping, words, words, text, off)
        assert (ids >= 0).sum() >= 6


# ------------------------------------------------------------------- 4: the families as whole documents
@pytest.mark.gpu
def test_families_as_documents(gpu, folds):
    """The max_word cases, the vanishing runes and every other family of tests/fold.py as tokens of small documents, one
    run per family on ONE batch."""
    import datok_amd
    tok = gpu(MODEL)
    made = {id(HAND): folds["hand"][1], id(HAND_REPL_VANISHES): folds["hand_repl_vanishes"][1]}
    with _B()(4096, 16) as b:
        for name, mapping, words, prefix, cases in fold.FAMILIES:
            assert prefix == b"##"
            keys = [k for k, _ in cases]
            docs = [b"Der " + k + b" ist da." for k in keys] + [b"", b" und ".join(keys)]
            vocab = datok_amd.Vocab(words)
            text, off, _ = _run(b, tok, docs, made[id(mapping)], vocab, vocab)
            ids, p, got_keys = _assert_folded(b, mapping, words, words, text, off)
            r = b.result()
            for key, expected in cases:
                i = got_keys.index(key)
                a, z = int(p.piece_off[i]), int(p.piece_off[i + 1])
                exp = fold.family_pieces(words, expected)
                assert p.piece_id[a:z].tolist() == [w for w, _ in exp], (name, key)
                assert (p.piece_bend[a:z].astype(np.int64) - int(r.tok_bstart[i])).tolist() == [e for _, e in exp], (name, key)
                assert int(p.piece_bend[z - 1]) == int(r.tok_bend[i])


# ------------------------------------------------------------------------------------------------- 5: staleness
@pytest.mark.gpu
def test_setting_a_fold_makes_the_finished_run_stale(gpu, folds):
    """Run, read pieces and ids, set_fold: both change without a new run; set_fold(None): both are the unfolded results
    again; the empty mapping gives what no fold gives; and the rows follow their pieces."""
    import datok_amd
    tok = gpu(MODEL)
    mapping, f = folds["hand"]
    id_words, wp_words = _vocabularies(mapping, POOL)
    id_vocab, wp_vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(wp_words)
    with _B()(8192, 16) as b:
        text, off, _ = _run(b, tok, _mixed_docs(70), None, id_vocab, wp_vocab)
        b.set_encode(8, 1, 2, 0, unit="document")
        ids0, p0, _ = _assert_folded(b, None, id_words, wp_words, text, off)
        rows0 = b.encoded().input_ids.copy()
        b.set_fold(f)
        ids1, p1, _ = _assert_folded(b, mapping, id_words, wp_words, text, off)
        assert not np.array_equal(ids0, ids1) and not np.array_equal(p0.piece_id, p1.piece_id)
        rows1 = b.encoded()
        e = datok_amd.encode_rows(p1.piece_off, p1.piece_id, [t1 for _, t1, _ in encode.units_of_documents(b.result().tok_off)],
                                  8, 1, 2, 0)
        assert np.array_equal(rows1.input_ids, e.input_ids)
        assert rows1.input_ids.shape != rows0.shape or not np.array_equal(rows1.input_ids, rows0)
        b.set_fold(None)
        ids2, p2, _ = _assert_folded(b, None, id_words, wp_words, text, off)
        assert np.array_equal(ids2, ids0) and np.array_equal(p2.piece_id, p0.piece_id) and np.array_equal(p2.piece_bend, p0.piece_bend)
        assert np.array_equal(b.encoded().input_ids, rows0)
        b.set_fold(folds["empty"][1])
        ids3, p3, _ = _assert_folded(b, {}, id_words, wp_words, text, off)
        assert np.array_equal(ids3, ids0) and np.array_equal(p3.piece_off, p0.piece_off) and np.array_equal(p3.piece_id, p0.piece_id)
        assert np.array_equal(p3.piece_bend, p0.piece_bend) and (p3.n_pieces, p3.n_unknown) == (p0.n_pieces, p0.n_unknown)
        b.set_fold(f)                                                   # a new run under the fold that is attached
        b.run(tok, 0)
        ids4, p4, _ = _assert_folded(b, mapping, id_words, wp_words, text, off)
        assert np.array_equal(ids4, ids1) and np.array_equal(p4.piece_id, p1.piece_id)


# --------------------------------------------------------------------------------------------------- 6: the chain
def _corpus_vocabularies(mapping, raw_words):
    keys = sorted({w for w in raw_words if _valid(w)})
    return _vocabularies(mapping, keys)


def _valid(w):
    try:
        w.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.gpu
def test_rows_behind_a_folded_split_and_a_tally(gpu, folds):
    """set_encode(max_len=8, sentences, word_ids) behind a folded split equals encode_rows over the folded pieces, and a
    tally under the fold holds the counts of the definition's ids."""
    import datok_amd
    tok = gpu(MODEL)
    mapping, f = folds["bert"]
    docs = _pipeline_documents()[:4] + [b" ".join(POOL), b""]
    id_words, wp_words = _corpus_vocabularies(mapping, [w for d in docs for w in d.split()])
    id_vocab, wp_vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(wp_words)
    tally = datok_amd.Tally(id_vocab)
    with _B()(1 << 16, 8) as b:
        b.set_encode(8, 1, 2, 0, unit="sentence", word_ids=True)
        text, off, _ = _run(b, tok, docs, f, id_vocab, wp_vocab, tally=tally)
        ids, p, keys = _assert_folded(b, mapping, id_words, wp_words, text, off)
        assert 2 * int((ids >= 0).sum()) > len(ids) and (np.diff(p.piece_off.astype(np.int64)) > 1).sum() > 50
        assert np.array_equal(tally.read(), tokenids.expected_counts(id_words, ids))
        r, sen, got = b.result(), b.sentences(), b.encoded()
        units = encode.units_of_sentences(r.tok_off, sen.sen_off, sen.sen_tok_end)
        exp = datok_amd.encode_rows(p.piece_off, p.piece_id, [t1 for _, t1, _ in units], 8, 1, 2, 0, word_ids=True, tok_off=r.tok_off)
        assert (got.n_units, got.n_rows, got.n_cut) == (exp.n_units, exp.n_rows, exp.n_cut) and got.n_rows > got.n_units > 10
        for k in ("unit_row_off", "input_ids", "row_len", "row_piece0", "word_id"):
            assert np.array_equal(getattr(got, k), getattr(exp, k)), k


@pytest.mark.gpu
def test_pipeline_and_stream_under_a_fold(gpu, folds):
    """A pipeline of at least three slices and a stream of at least three deliver, joined, the single batch's folded ids
    and pieces."""
    import datok_amd
    from datok_amd import corpus
    tok = gpu(MODEL)
    mapping, f = folds["bert"]
    docs = _pipeline_documents()[:20]
    id_words, wp_words = _corpus_vocabularies(mapping, [w for d in docs for w in d.split()])
    id_vocab, wp_vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(wp_words)
    text, off = corpus.concat_docs(docs)
    with _B()(len(text), len(docs)) as b:
        _run(b, tok, docs, f, id_vocab, wp_vocab)
        ids1, p1, _ = _assert_folded(b, mapping, id_words, wp_words, text, off)
        b.set_fold(None)
        assert not np.array_equal(b.token_ids()[0], ids1)               # (the fold matters on this text)
    got = []

    def on_slice(first, n, bb):
        got.append((bb.token_ids()[0], bb.pieces()))
    with datok_amd.Pipeline(12 << 10, 64, depth=3) as p:
        p.set_vocab(id_vocab)
        p.set_wordpiece(wp_vocab)
        p.set_fold(f)
        p.run(tok, text, off, 0, on_slice)
        assert len(got) >= 3
        assert np.array_equal(np.concatenate([g[0] for g in got]), ids1)
        assert np.array_equal(np.concatenate([g[1].piece_id for g in got]), p1.piece_id)
        assert np.array_equal(np.concatenate([g[1].piece_bend for g in got]), p1.piece_bend)
        assert sum(g[1].n_unknown for g in got) == p1.n_unknown
        p.set_fold(None)
    raw = streamcorpus.running_text(64 << 10, seed=11)
    id_words, wp_words = _corpus_vocabularies(mapping, raw.split())
    id_vocab, wp_vocab = datok_amd.Vocab(id_words), datok_amd.Vocab(wp_words)
    with _B()(len(raw), 1) as b:
        _run(b, tok, [raw], f, id_vocab, wp_vocab)
        ids1, p1, _ = _assert_folded(b, mapping, id_words, wp_words, *corpus.concat_docs([raw]))
    slices = []
    with datok_amd.Stream(streamcorpus.S) as s:
        s.set_vocab(id_vocab)
        s.set_wordpiece(wp_vocab)
        s.set_fold(f)
        assert s.run(tok, raw, 0, slices.append) == 0
        streamcorpus.check_slices(slices, len(raw))
        assert len(slices) >= 3
        assert np.array_equal(np.concatenate([sl.tok_id for sl in slices]), ids1)
        assert np.array_equal(np.concatenate([sl.piece_id for sl in slices]), p1.piece_id)
        ends = np.concatenate([sl.piece_bend.astype(np.int64) + sl.base for sl in slices])
        assert np.array_equal(ends, p1.piece_bend.astype(np.int64))
        s.set_fold(None)


# --------------------------------------------------------------------------------------------------- 7: errors
@pytest.mark.gpu
def test_errors(gpu, folds):
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    with _B()(1024, 2) as b:
        assert L.dtk_batch_set_fold(None, None) == _lib.E_ARG
        b.set_fold(folds["hand"][1])
        b.set_fold(None)
    with pytest.raises(_lib.DatokGpuError) as e:
        datok_amd.Fold({0xD800: "a"})
    assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.DatokGpuError) as e:
        datok_amd.Fold({0x41: "aaaaa"})
    assert e.value.code == _lib.E_ARG
