"""Tokenizers of 32 767 states and more: the 64-bit fused cells (dtk_model.cpp pick_encoding, FusedCell64 in
dtk_walk_core.h) against the CPU oracle, bit exact, every document of every corpus compared in full.

No shipped model is that large; the models are made here (tests/wide.py): real models with their states scattered
over more ids -- the oracle's output for the ORIGINAL file is the expected value -- and a 65 541-state trie automaton
whose expected values are those of craft.matok() / craft.datok().
"""
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import craft
import wide
from conftest import MODELS, ROOT
from parity import FIELDS, assert_batch_equals_oracle

NEWLINE_AFTER_EOT = 16
SIMPLE, TOKEN_POS = 3, 4
WIDENED = [("tokenizer_de.matok", 40000), ("tokenizer_en.matok", 40000)]


def _read(name):
    with open(os.path.join(MODELS, name), "rb") as f:
        return f.read()


def _oracle(blob):
    from oracle import oracle as O
    return O.Model(raw=gzip.decompress(blob))


_widened = {}


def _widened_blob(name, n_states):
    if (name, n_states) not in _widened:
        _widened[(name, n_states)] = wide.widen_matok(_read(name), n_states)
    return _widened[(name, n_states)]


def _same_on_oracle(oa, ob, doc, flags, events=False):
    ra, rb = oa.transduce_doc(doc, flags), ob.transduce_doc(doc, flags)
    for f in FIELDS:
        assert np.array_equal(getattr(ra, f), getattr(rb, f)), (f, flags, doc[:80])
    assert ra.status == rb.status, (flags, doc[:80])
    if events:
        assert oa.events(doc) == ob.events(doc), doc[:80]


# ------------------------------------------------------------------------------------------------ CPU tier
def test_widened_model_is_the_same_tokenizer_on_the_oracle(oracle_models):
    """The yardstick: scattering the states changes nothing the reference computes."""
    from datok_amd import corpus
    text, off = corpus.german_docs(64, 4096, seed=3)
    raw = text.tobytes()
    a, b = oracle_models("tokenizer_de.matok"), _oracle(_widened_blob("tokenizer_de.matok", 40000))
    for d in range(64):
        _same_on_oracle(a, b, raw[int(off[d]):int(off[d + 1])], 0)


@pytest.mark.parametrize("kind", ["matok", "datok"])
def test_trie_model_is_the_crafted_tokenizer_on_the_oracle(kind):
    """... and unfolding the word state into 65 536 trie nodes changes nothing either: arrays, status, call list."""
    a, b = _oracle(getattr(craft, kind)()), _oracle(wide.trie_model(kind))
    docs = craft.documents(np.random.default_rng(5), n=400, max_len=200)
    assert len(docs) == 416
    for doc in docs:
        for flags in (0, NEWLINE_AFTER_EOT):
            _same_on_oracle(a, b, doc, flags, events=flags == 0)


def _info_in_child(tmp_path, blob, env):
    """datok_amd.model_info(blob) in a process of its own with `env` added (the test hooks are read once per process)."""
    path = tmp_path / "image.gz"
    path.write_bytes(blob)
    code = ("import sys, json; sys.path.insert(0, %r); import datok_amd; "
            "print(json.dumps(datok_amd.model_info(open(%r, 'rb').read())))" % (ROOT, str(path)))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    import json
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def test_model_info_without_a_device(tmp_path):
    """dtk_model_info_mem: which table a model file gets, decided as the loader decides it, on a machine without a GPU."""
    import datok_amd
    from datok_amd import _lib
    if any(os.environ.get(k) for k in ("DATOK_NO_FUSED", "DATOK_FORCE_WIDE", "DATOK_NO_DENSE", "DATOK_WIDE_FUSED")):
        pytest.skip("the switches that select other table encodings change these answers")
    de, de_da = _read("tokenizer_de.matok"), _read("tokenizer_de.datok")
    widened = _widened_blob("tokenizer_de.matok", 40000)
    orig, w = datok_amd.model_info(de), datok_amd.model_info(widened)
    assert (w["kind"], w["state_count"], w["entry_bytes"]) == (0, 40000, 8), w
    assert w["stream_codes"] == orig["stream_codes"] and orig["stream_codes"] > 0
    assert w["n_eps_states"] == orig["n_eps_states"] and w["unknown_used"] == orig["unknown_used"] == 0
    assert w["device_bytes"] > 40001 * 176 * 8          # rows of 176 cells of 8 bytes
    assert (orig["kind"], orig["state_count"], orig["entry_bytes"], orig["dense_states"]) == (0, 18400, 4, 0), orig
    da = datok_amd.model_info(de_da)
    assert da["kind"] == 1 and da["dense_states"] > 0 and da["entry_bytes"] == 4, da
    t = datok_amd.model_info(wide.trie_model("datok"))
    assert (t["kind"], t["dense_states"], t["entry_bytes"]) == (1, wide.TRIE_STATES, 8), t
    t = datok_amd.model_info(wide.trie_model("matok"))
    assert (t["kind"], t["state_count"], t["entry_bytes"], t["dense_states"]) == (0, wide.TRIE_STATES, 8, 0), t
    # the test hooks keep their meaning: plain cells for the large model as before, 64-bit fused cells for a small one
    assert _info_in_child(tmp_path, widened, {"DATOK_NO_FUSED": "1"})["entry_bytes"] == 4
    assert _info_in_child(tmp_path, widened, {"DATOK_FORCE_WIDE": "1"})["entry_bytes"] == 4
    assert _info_in_child(tmp_path, de, {"DATOK_WIDE_FUSED": "1"})["entry_bytes"] == 8
    assert _info_in_child(tmp_path, de, {"DATOK_NO_FUSED": "1"})["entry_bytes"] == 2
    da = _info_in_child(tmp_path, wide.trie_model("datok"), {"DATOK_NO_DENSE": "1"})
    assert (da["dense_states"], da["entry_bytes"]) == (0, 8)          # the {base, check} pairs
    da = _info_in_child(tmp_path, wide.trie_model("datok"), {"DATOK_NO_FUSED": "1"})
    assert (da["dense_states"], da["entry_bytes"]) == (0, 8)
    # images the loader rejects
    for bad in (de[:len(de) // 2], gzip.compress(gzip.decompress(de)[:100000]), gzip.compress(b"MATOK"), b"", b"junk" * 10):
        with pytest.raises(datok_amd.DatokGpuError) as e:
            datok_amd.model_info(bad)
        assert e.value.code == _lib.E_FORMAT, bad[:20]
    # the C-ABI itself: null arguments
    info = _lib.ModelInfo()
    assert datok_amd.lib().dtk_model_info_mem(None, 0, info) == _lib.E_ARG


def test_cpp_mirror_model_info(tmp_path):
    """datok::ModelInfo (include/datok.hpp) over the same entry point."""
    src = tmp_path / "info.cpp"
    src.write_text(r"""
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>
#include "datok.hpp"
int main(int argc, char **argv) {
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  dtk_model_info i;
  if (!datok::ModelInfo(b.data(), b.size(), &i)) return 3;
  std::printf("%d %u %u %u\n", i.kind, i.state_count, i.entry_bytes, i.dense_states);
  return datok::ModelInfo(b.data(), b.size() / 2, &i) ? 4 : 0;
}
""")
    exe = tmp_path / "info"
    libdir = os.path.join(ROOT, "datok_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldatok_gpu", "-Wl,-rpath," + libdir])
    img = tmp_path / "trie.datok"
    img.write_bytes(wide.trie_model("datok"))
    e = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
    r = subprocess.run([str(exe), str(img)], capture_output=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    assert r.stdout.decode().split() == ["1", "720948", "8", str(wide.TRIE_STATES)]


# ------------------------------------------------------------------------------------------------ GPU tier
def _forced():
    return any(os.environ.get(k) for k in ("DATOK_NO_FUSED", "DATOK_FORCE_WIDE"))


@pytest.fixture(scope="module")
def load(tmp_path_factory):
    """blob -> Tokenizer (through a file, as LoadTokenizerFile takes it), cached by name."""
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache, where = {}, tmp_path_factory.mktemp("wide_models")

    def get(name, blob):
        if name not in cache:
            path = where / name
            path.write_bytes(blob)
            cache[name] = datok_amd.load_tokenizer_file(str(path))
            assert cache[name] is not None, name
        return cache[name]
    return get


def _widened_tok(load, name, n_states):
    tok = load("%s.wide%d" % (name, n_states), _widened_blob(name, n_states))
    if not _forced():
        assert tok.info["entry_bytes"] == 8 and tok.info["state_count"] == n_states, tok.info
    return tok


def _run(tok, text, off, flags=0, chunk=None, warm=64):
    import datok_amd
    with datok_amd.Batch(max(len(text), 1), len(off) - 1) as b:
        if chunk is not None:
            b.set_chunking(chunk, warm, extend=0 if warm < 16 else None)
        b.set_input(text, off)
        b.run(tok, flags)
        return b.result(), b.totals()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_states", WIDENED)
def test_widened_model_gets_64bit_fused_cells(load, name, n_states):
    if _forced():
        pytest.skip("DATOK_NO_FUSED / DATOK_FORCE_WIDE select the plain cells")
    tok = _widened_tok(load, name, n_states)
    orig = __import__("datok_amd").model_info(_read(name))
    assert tok.info["entry_bytes"] == 8 and tok.info["kind"] == 0 and tok.info["dense_states"] == 0
    assert tok.info["stream_codes"] == orig["stream_codes"] and tok.info["n_eps_states"] == orig["n_eps_states"]
    assert tok.info == __import__("datok_amd").model_info(_widened_blob(name, n_states))   # the host-only answer
    assert tok.type() == "MATOK"


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_states", WIDENED)
@pytest.mark.parametrize("chunk,warm", [(None, 64), (0, 64), (64, 64), (128, 64), (256, 64), (64, 0), (128, 4), (256, 0)])
def test_widened_model_german_docs(load, oracle_models, name, n_states, chunk, warm):
    """The lean loop over 64-bit cells: one lane per document, speculative chunks, repair rounds (warm-ups 0 / 4 with
    no help from the previous blank)."""
    from datok_amd import corpus
    text, off = corpus.german_docs(256, 4096, seed=13)
    res, tot = _run(_widened_tok(load, name, n_states), text, off, chunk=chunk, warm=warm)
    assert tot["n_flagged"] == 0 and tot["n_texts"] == 256
    if chunk:
        assert tot["chunk_bytes"] == chunk and tot["n_lanes"] > 256
    if chunk and warm == 0:
        assert tot["repair_rounds"] > 0
    assert assert_batch_equals_oracle(oracle_models(name), res, text, off) == 256


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_states", WIDENED)
def test_widened_model_rich_edge_and_eot_documents(load, oracle_models, name, n_states):
    """The rich corpus, the raw-byte / edge documents, and long documents stuffed with EOT texts, with and without
    NEWLINE_AFTER_EOT."""
    import datok_amd
    from datok_amd import corpus
    from test_gpu_parity import _edge_docs
    tok, om = _widened_tok(load, name, n_states), oracle_models(name)
    text, off = corpus.german_rich_docs(192, 4096, seed=4)
    res, tot = _run(tok, text, off)
    assert assert_batch_equals_oracle(om, res, text, off) == 192
    edge = _edge_docs()
    text, off = corpus.concat_docs(edge)
    for flags, chunk, warm in ((0, 0, 64), (NEWLINE_AFTER_EOT, 0, 64), (0, 16, 64), (NEWLINE_AFTER_EOT, 32, 8), (0, 64, 0)):
        res, tot = _run(tok, text, off, flags, chunk=chunk, warm=warm)
        assert not any(int(s) & datok_amd.ST_IRREGULAR for s in res.status)
        assert assert_batch_equals_oracle(om, res, text, off, flags) > 200     # (as test_edge_documents)
    rng = np.random.default_rng(99)
    docs = []
    for k in range(4):
        parts = [edge[int(i)] for i in rng.integers(0, len(edge), size=int(rng.integers(200, 500)))]
        sep = [b" ", b"\n", b"\x04", b"\x04\n", b". ", b"\x04\x04"]
        raw = b"".join(p + sep[int(rng.integers(0, len(sep)))] for p in parts if len(p) < 400)
        docs.append((b"\x04\x04" + raw) if k == 0 else (raw + b"\x04") if k == 1 else raw)
    text, off = corpus.concat_docs(docs)
    for flags, chunk in ((0, 48), (NEWLINE_AFTER_EOT, 128), (NEWLINE_AFTER_EOT, None), (0, 0)):
        res, tot = _run(tok, text, off, flags, chunk=chunk, warm=48)
        assert_batch_equals_oracle(om, res, text, off, flags)


@pytest.mark.gpu
def test_widened_model_one_long_document(load, oracle_models):
    """One 8 MiB document: thousands of lanes, compacted in segments."""
    from datok_amd import corpus
    text, _ = corpus.german_docs(2048, 4096, seed=21)
    assert len(text) == 8 << 20
    off = np.array([0, len(text)], dtype=np.uint64)
    res, tot = _run(_widened_tok(load, "tokenizer_de.matok", 40000), text, off)
    assert tot["n_lanes"] > 4096 and tot["n_flagged"] == 0
    assert assert_batch_equals_oracle(oracle_models("tokenizer_de.matok"), res, text, off) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_states", WIDENED)
def test_widened_model_rendering_and_single_stream(load, oracle_models, name, n_states):
    """NewTokenWriter's bytes rendered on the device (SIMPLE and a position mode), and one reader through
    Tokenizer.transduce_token_writer / transduce_bytes (the per-thread batch, closures replayed)."""
    import datok_amd
    from datok_amd import corpus
    tok, om = _widened_tok(load, name, n_states), oracle_models(name)
    text, off = corpus.german_docs(256, 4096, seed=17)
    raw = text.tobytes()
    with datok_amd.Batch(len(text), 256) as b:
        b.set_input(text, off)
        b.run(tok, 0)
        for bits in (SIMPLE, TOKEN_POS, 15):
            data, o = b.render(bits)
            for d in range(256):
                exp, est = om.transduce(raw[int(off[d]):int(off[d + 1])], bits)
                assert est == 0 and data[int(o[d]):int(o[d + 1])] == exp, (bits, d)
    one = "Der Vorsitzende der Abk. hat gewählt. „Zitat“ – so … Gefunden auf wikipedia.org.\x04\nUnd weiter.".encode()
    w = io.BytesIO()
    assert tok.transduce_token_writer(io.BytesIO(one), datok_amd.new_token_writer(w, SIMPLE))
    assert w.getvalue() == om.transduce(one, SIMPLE)[0]
    for bits in (SIMPLE, 15 | NEWLINE_AFTER_EOT):
        assert tok.transduce_bytes(one, bits) == (om.transduce(one, bits)[0], 0)
        assert tok.transduce_bytes(one, bits, replay=True) == (om.transduce(one, bits)[0], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,triple", [("matok", False), ("datok", False), ("matok", True), ("datok", True)])
def test_trie_models_equal_the_oracle(load, kind, triple):
    """65 541 states, all reachable, high ids in every word: arrays, status, the calls of the documents that went
    through the exact pass (the double array's EOT read twice; three SentenceEnds at one cursor), rendered bytes."""
    import datok_amd
    from datok_amd import corpus
    from test_exact_and_replay import _oracle_calls, _replayed
    blob = wide.trie_model(kind, triple)
    tok, om = load("trie%d.%s" % (triple, kind), blob), _oracle(getattr(craft, kind)(triple))
    assert tok.type() == kind.upper()
    if not _forced() and not os.environ.get("DATOK_NO_DENSE"):
        assert tok.info["entry_bytes"] == 8, tok.info
        n_states = wide.TRIE_STATES + (2 if triple else 0)
        assert tok.info["dense_states"] == (n_states if kind == "datok" else 0), tok.info
        assert kind == "datok" or tok.info["state_count"] == n_states
    docs = craft.documents(np.random.default_rng(5), n=400, max_len=200)
    text, off = corpus.concat_docs(docs)
    for chunk, flags in ((0, 0), (16, NEWLINE_AFTER_EOT), (None, 0), (64, 0)):
        with datok_amd.Batch(max(len(text), 1), len(docs)) as b:
            if chunk is not None:
                b.set_chunking(chunk, 8, extend=0)
            b.set_input(text, off)
            b.run(tok, flags)
            res = b.result()
            assert not any(int(s) & datok_amd.ST_IRREGULAR for s in res.status)
            # (every document is compared; the count is of those the reference does not panic on: long random
            #  documents mostly hold a text without a token)
            assert assert_batch_equals_oracle(om, res, text, off, flags) > 0
            if kind == "datok" or triple:
                assert len(res.exact) > 0        # the construct occurred: the exact pass ran over the wide cells
            for d, doc in enumerate(docs):
                exp = [c[:3] if c[0] == "T" else c for c in _oracle_calls(om, doc)]
                assert _replayed(res, d, doc, kind == "matok") == exp, (d, doc)
            for bits in (3, 15):
                data, o = b.render(bits | flags)
                for d, doc in enumerate(docs):
                    exp, est = om.transduce(doc, bits | flags)
                    if est == 0 and not (int(res.status[d]) & ~datok_amd.ST_EMPTY_TEXT):
                        assert data[int(o[d]):int(o[d + 1])] == exp, (bits, d, doc)


@pytest.mark.gpu
def test_general_loop_over_wide_cells_random_automata(load):
    """Random arc tables (they carry arcs on `unknown` and `identity`: the general loop, walk_lane) widened to 33 000
    states, against the oracle on the widened image."""
    import datok_amd
    from datok_amd import corpus
    compared = with_unknown = 0
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        arcs = craft.random_automaton(rng)
        blob = wide.widen_matok(craft.matok_from(arcs), 33000, seed=seed)
        docs = craft.random_documents(rng) + [b" \x04", b"a \x04", b"bx \nb\x04", b"\n", b"\n\n"]
        text, off = corpus.concat_docs(docs)
        tok, om = load("random%d.matok" % seed, blob), _oracle(blob)
        if not _forced():
            assert tok.info["entry_bytes"] == 8 and tok.info["state_count"] == 33000, tok.info
        with_unknown += tok.info["unknown_used"]
        for chunk, warm in ((0, 0), (16, 0), (32, 4), (None, 16)):
            for flags in (0, NEWLINE_AFTER_EOT):
                with datok_amd.Batch(len(text), len(docs)) as b:
                    if chunk is not None:
                        b.set_chunking(chunk, warm, extend=0 if warm < 8 else 16)
                    b.set_input(text, off)
                    b.run(tok, flags)
                    res = b.result()
                    try:
                        compared += assert_batch_equals_oracle(om, res, text, off, flags)
                    except AssertionError as e:
                        raise AssertionError("seed %d chunk %r warm %d flags %d: %s" % (seed, chunk, warm, flags, e))
                    if chunk == 0:
                        data, o = b.render(3 | flags)
                        for d, doc in enumerate(docs):
                            exp, est = om.transduce(doc, 3 | flags)
                            if est == 0 and not (int(res.status[d]) & ~datok_amd.ST_EMPTY_TEXT):
                                assert bytes(data[int(o[d]):int(o[d + 1])]) == exp, (seed, flags, doc)
    assert compared > 0 and with_unknown > 0     # some of them do walk the general loop


@pytest.mark.gpu
def test_general_loop_over_wide_cells_clitic_model(load, oracle_models):
    """clitic_test.matok widened to 33 000 states on the inputs its goldens use (the failure ladder with the
    `unknown` retry, matrix.go:478-485) and on the edge documents."""
    from datok_amd import corpus
    from goldens import load_cases
    from test_gpu_parity import _edge_docs
    tok, om = _widened_tok(load, "clitic_test.matok", 33000), oracle_models("clitic_test.matok")
    inputs = sorted({c["input"] for case in load_cases() for c in case["calls"] if c["model"] == "clitic_test.matok"})
    assert inputs
    for s in inputs:
        for bits in (SIMPLE, 15):
            exp, est = om.transduce(s.encode(), bits)
            if est == 0:
                assert tok.transduce_bytes(s.encode(), bits) == (exp, 0), s
    docs = [s.encode() for s in inputs] + _edge_docs()
    text, off = corpus.concat_docs(docs)
    for flags, chunk, warm in ((0, 0, 64), (NEWLINE_AFTER_EOT, 16, 64), (0, 32, 0), (0, None, 64)):
        res, _ = _run(tok, text, off, flags, chunk=chunk, warm=warm)
        assert assert_batch_equals_oracle(om, res, text, off, flags) > 200


_CHILD_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import datok_amd
from datok_amd import corpus
from oracle import oracle as O
from parity import assert_batch_equals_oracle
tok = datok_amd.load_tokenizer_file(sys.argv[2])
assert tok is not None and tok.info["state_count"] == 40000 and tok.info["entry_bytes"] == int(sys.argv[3]), tok.info
om = O.Model(os.path.join(sys.argv[1], "tests", "golden", "models", "tokenizer_de.matok"))
text, off = corpus.german_docs(256, 4096, seed=13)
for chunk, warm in ((None, 64), (0, 64), (128, 4)):
    with datok_amd.Batch(len(text), 256) as b:
        if chunk is not None:
            b.set_chunking(chunk, warm, extend=0 if warm < 16 else None)
        b.set_input(text, off); b.run(tok, 0)
        res, tot = b.result(), b.totals()
        assert tot["n_flagged"] == 0
        assert assert_batch_equals_oracle(om, res, text, off) == 256
print("CHILD OK")
"""


@pytest.mark.gpu
def test_plain_cells_for_a_large_model_still_work(tmp_path):
    """DATOK_NO_FUSED=1: the widened model on plain 32-bit cells and the general loop -- the path every model of
    32 767 states and more took before the 64-bit cells."""
    script, img = tmp_path / "child.py", tmp_path / "wide.matok"
    script.write_text(_CHILD_SCRIPT)
    img.write_bytes(_widened_blob("tokenizer_de.matok", 40000))
    e = dict(os.environ)
    e["DATOK_NO_FUSED"] = "1"
    r = subprocess.run([sys.executable, str(script), ROOT, str(img), "4"], capture_output=True, env=e, timeout=600)
    assert r.returncode == 0 and b"CHILD OK" in r.stdout, r.stderr.decode()[-2000:]


@pytest.mark.gpu
def test_existing_suite_over_64bit_cells():
    """DATOK_WIDE_FUSED=1 lays every model out in 64-bit fused cells: the goldens through the C-ABI, exact pass and
    replay, edge documents, speculative chunks, random automata and the double-array tests in a process of their own.
    (Left out: the tests that assert a cell size of 4, and this file.)"""
    if any(os.environ.get(k) for k in ("DATOK_NO_FUSED", "DATOK_FORCE_WIDE", "DATOK_NO_DENSE", "DATOK_WIDE_FUSED")):
        pytest.skip("already running under a switch that selects a table encoding")
    e = dict(os.environ)
    e["DATOK_WIDE_FUSED"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "(goldens_through or out_of_position or closure_int or edge_documents or speculative_chunks or "
                        "random_automata or datok or double_array or config4 or rich_corpus or long_documents) and not "
                        "pairs_path and not type_and_loader and not wide_models", os.path.join(ROOT, "tests")],
                       capture_output=True, env=e, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-500:])
    assert b" passed" in r.stdout
