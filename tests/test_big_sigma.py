"""Tokenizers with more than 255 distinct symbol-stream entries: the lean loop over 16-bit entries (WinEntries in
dtk_walk_core.h; `dtk_model_info.lean_walk`) against the CPU oracle, bit exact, every document compared in full.

No shipped model has that many entries; the models are made here (tests/bigsigma.py): `tokenizer_de.matok` with more
characters in its sigma -- the oracle's output for the enlarged file is the expected value, and on text without the
new characters it is the original file's, which the reference's goldens pin -- and craft's automata over a sigma with
300 more characters.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import bigsigma
import craft
import wide
from conftest import ROOT
from parity import FIELDS, assert_batch_equals_oracle

NEWLINE_AFTER_EOT = 16
SWITCHES = ("DATOK_NO_FUSED", "DATOK_FORCE_WIDE", "DATOK_NO_DENSE", "DATOK_GENERAL16")


def _switched():
    return any(os.environ.get(k) for k in SWITCHES)


# ------------------------------------------------------------------------------------------------ CPU tier
def test_enlarged_model_is_the_original_on_text_without_the_new_characters(oracle_models):
    """The yardstick: on documents without the new characters the oracle gives the same offsets and the same rendered
    bytes for the enlarged file and for the original, which the goldens pin."""
    from datok_amd import corpus
    a, b = oracle_models("tokenizer_de.matok"), bigsigma.oracle_of(bigsigma.enlarged_de(64))
    text, off = corpus.german_docs(48, 4096, seed=3)
    raw = text.tobytes()
    docs = [raw[int(off[d]):int(off[d + 1])] for d in range(48)]
    docs += ["Der Vorsitzende der Abk. hat gewählt. „Zitat“ – so … z. B. 1.000 Euro.\x04\nUnd weiter.".encode(), b"", b"\x04"]
    for doc in docs:
        ra, rb = a.transduce_doc(doc, 0), b.transduce_doc(doc, 0)
        for f in FIELDS:
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), (f, doc[:80])
        assert ra.status == rb.status
        for bits in (3, 15):
            assert a.transduce(doc, bits) == b.transduce(doc, bits), (bits, doc[:80])


def test_new_characters_act_like_their_models_on_the_oracle():
    """... and a new character is tokenised like the character whose column it got: same token and sentence counts
    with the new characters put back to "a", "." and " "."""
    om = bigsigma.oracle_of(bigsigma.enlarged_de(64))
    text, off, docs = bigsigma.german_spliced()
    back = {ord(c): l for c, l in zip(bigsigma.CHARS, bigsigma.LIKE)}
    n_new = 0
    for doc in docs[:16]:
        s = doc.decode("utf-8")
        n_new += sum(1 for c in s if ord(c) in back)
        ra, rb = om.transduce_doc(doc, 0), om.transduce_doc(s.translate(back).encode("utf-8"), 0)
        assert ra.status == rb.status == 0
        for f in ("tok_rstart", "tok_rend", "sent", "text_tok_end", "text_sent_end"):   # (rune offsets: the widths differ)
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), (f, doc[:80])
    assert n_new > 16 * 100          # (the documents do carry them: about one per 25 bytes)


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
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def test_model_info_tells_which_loop(tmp_path):
    """dtk_model_info.lean_walk, decided on the host: the stream's format (`stream_codes`) no longer decides the loop."""
    import datok_amd
    if _switched() or any(os.environ.get(k) for k in ("DATOK_SYM16", "DATOK_WIDE_FUSED")):
        pytest.skip("the switches that select other encodings or loops change these answers")
    de = bigsigma.read_model("tokenizer_de.matok")
    i = datok_amd.model_info(de)
    assert (i["sigma_count"], i["stream_codes"], i["lean_walk"], i["unknown_used"]) == (171, 202, 1, 0), i
    i = datok_amd.model_info(bigsigma.enlarged_de(53))
    assert (i["sigma_count"], i["stream_codes"], i["lean_walk"]) == (224, 255, 1), i      # the last model that fits the codes
    for k in (54, 64):
        i = datok_amd.model_info(bigsigma.enlarged_de(k))
        assert (i["sigma_count"], i["stream_codes"], i["entry_bytes"]) == (171 + k, 0, 4), i
        assert i["lean_walk"] == 1, i           # 16-bit entries AND the lean loop
    assert _info_in_child(tmp_path, bigsigma.enlarged_de(64), {"DATOK_GENERAL16": "1"})["lean_walk"] == 0
    assert _info_in_child(tmp_path, de, {"DATOK_GENERAL16": "1"})["lean_walk"] == 1      # (codes: the hook does not apply)
    i = _info_in_child(tmp_path, de, {"DATOK_SYM16": "1"})
    assert (i["stream_codes"], i["lean_walk"]) == (0, 1), i
    assert _info_in_child(tmp_path, de, {"DATOK_NO_FUSED": "1"})["lean_walk"] == 0       # plain cells: the general loop
    # an arc on `unknown`: the general loop, whatever the stream
    arcs = craft._automaton(False)
    arcs[1][craft.UNKNOWN] = (2, False)
    i = datok_amd.model_info(craft.matok_from(arcs))
    assert (i["unknown_used"], i["lean_walk"]) == (1, 0) and i["stream_codes"] > 0, i
    i = datok_amd.model_info(craft.matok())
    assert (i["unknown_used"], i["lean_walk"]) == (0, 1), i
    # 64-bit cells with entries
    i = datok_amd.model_info(wide.widen_matok(bigsigma.enlarged_de(64), 40000))
    assert (i["entry_bytes"], i["stream_codes"], i["lean_walk"], i["state_count"]) == (8, 0, 1, 40000), i
    # a double array: the lean loop walks its dense layout, the general loop its pairs
    for blob in (craft.big_sigma("datok")[0], bigsigma.crafted("datok", True)[0]):
        i = datok_amd.model_info(blob)
        print("crafted .datok over 310 characters: dense_states %d stream_codes %d lean_walk %d" % (
            i["dense_states"], i["stream_codes"], i["lean_walk"]))
        assert i["kind"] == 1 and i["stream_codes"] == 0 and i["lean_walk"] == (1 if i["dense_states"] > 0 else 0), i
        assert i["dense_states"] > 0
    i = _info_in_child(tmp_path, craft.big_sigma("datok")[0], {"DATOK_NO_DENSE": "1"})
    assert (i["dense_states"], i["lean_walk"]) == (0, 0), i
    i = datok_amd.model_info(craft.big_sigma("matok")[0])
    assert (i["stream_codes"], i["lean_walk"]) == (0, 1), i


def test_model_info_struct_mirrors_the_header(tmp_path):
    """dtk_model_info of include/datok_gpu.h against datok_amd/_lib.py's ModelInfo: size and every offset."""
    from datok_amd import _lib
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "datok_gpu.h"', 'int main(void) {',
           'printf("size %zu\\n", sizeof(dtk_model_info));']
    for fname, _ in _lib.ModelInfo._fields_:
        src.append('printf("%s %%zu\\n", offsetof(dtk_model_info, %s));' % (fname, fname))
    src.append("return 0; }")
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.ModelInfo)
    for fname, _ in _lib.ModelInfo._fields_:
        assert int(got[fname]) == getattr(_lib.ModelInfo, fname).offset, fname
    assert _lib.ModelInfo._fields_[-1][0] == "lean_walk"


def test_cpp_mirror_tells_which_loop(tmp_path):
    """datok::ModelInfo (include/datok.hpp) over the same entry point prints the new member."""
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
  std::printf("%d %d %u %u %u\n", i.kind, i.sigma_count, i.entry_bytes, i.stream_codes, i.lean_walk);
  return 0;
}
""")
    exe = tmp_path / "info"
    libdir = os.path.join(ROOT, "datok_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-ldatok_gpu", "-Wl,-rpath," + libdir])
    img = tmp_path / "de64.matok"
    img.write_bytes(bigsigma.enlarged_de(64))
    e = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
    r = subprocess.run([str(exe), str(img)], capture_output=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    assert r.stdout.decode().split() == ["0", "235", "4", "0", "1"]


# ------------------------------------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def load(tmp_path_factory):
    """blob -> Tokenizer (through a file, as LoadTokenizerFile takes it), cached by name."""
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache, where = {}, tmp_path_factory.mktemp("big_sigma")

    def get(name, blob):
        if name not in cache:
            path = where / name
            path.write_bytes(blob)
            cache[name] = datok_amd.load_tokenizer_file(str(path))
            assert cache[name] is not None, name
            if not _switched():
                assert cache[name].info["stream_codes"] == 0 and cache[name].info["lean_walk"] == 1, cache[name].info
        return cache[name]
    return get


def _run(tok, text, off, flags=0, chunk=None, warm=64, render=None, batch=None):
    """(result, totals, rendered bytes per document or None)"""
    import datok_amd
    b = batch or datok_amd.Batch(max(len(text), 1), len(off) - 1)
    try:
        if chunk is not None:
            b.set_chunking(chunk, warm, extend=0 if warm < 16 else None)
        b.set_input(text, off)
        b.run(tok, flags)
        res, tot, out = b.result(), b.totals(), None
        if render is not None:
            data, o = b.render(render | flags)
            out = [bytes(data[int(o[d]):int(o[d + 1])]) for d in range(len(off) - 1)]
        return res, tot, out
    finally:
        if batch is None:
            b.close()


def _assert_rendered(om, rendered, res, docs, bits, flags=0):
    import datok_amd
    n = 0
    for d, doc in enumerate(docs):
        exp, est = om.transduce(doc, bits | flags)
        if est == 0 and not (int(res.status[d]) & ~datok_amd.ST_EMPTY_TEXT):
            assert rendered[d] == exp, (d, bits, flags, doc[:120])
            n += 1
    return n


CHUNKINGS = [(None, 64), (0, 64), (16, 4), (64, 0), (128, 4), (256, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,warm", CHUNKINGS)
def test_enlarged_model_german_docs(load, chunk, warm):
    """64 German documents of 4 KiB with the new characters inside words, as sentence ends and as blanks: one lane per
    document, speculative chunks, repair rounds (warm-ups 0 / 4 with no help from the previous blank)."""
    blob = bigsigma.enlarged_de(64)
    tok, om = load("de64.matok", blob), bigsigma.oracle_of(blob)
    text, off, docs = bigsigma.german_spliced()
    res, tot, out = _run(tok, text, off, chunk=chunk, warm=warm, render=3)
    assert tot["n_flagged"] == 0 and tot["n_texts"] == 64
    if chunk:
        assert tot["chunk_bytes"] == chunk and tot["n_lanes"] > 64
    if chunk and warm == 0:
        assert tot["repair_rounds"] > 0
    assert assert_batch_equals_oracle(om, res, text, off) == 64
    assert _assert_rendered(om, out, res, docs, 3) == 64


def _edge_items():
    l = bigsigma.LETTERS
    return [l[3].encode(), bigsigma.CHAR3.encode(), bigsigma.CHAR4.encode(), b"\x04", b"\xff", b"\xe4\xb8",
            bigsigma.OUTSIDE.encode(), "".join(l[i] for i in range(20)).encode()]


TRUNCATED = 5      # (index of the truncated rune in _edge_items)


def _edge_documents():
    """8 kinds of item at every document-relative position 0 .. bigsigma.EDGE_POSITIONS - 1, documents of 112 bytes;
    on top of them documents that end in the truncated rune; the whole set 16 times with a one-byte document between
    two sets, so that every document starts at every residue 0..15 of the stream.
    Returns (docs, [(kind, position of the item in the document built, residue of the document's start) or None per
    document]): the bookkeeping is read from the documents, not from the loops that made them."""
    filler = ("ab cd ef. gh " * 8).encode()
    tail = (" xy. Ende z. B. 1.000 da " * 6).encode()
    items = _edge_items()
    docs, where, at = [], [], 0

    def add(doc, k):
        nonlocal at
        docs.append(doc)
        where.append(None if k is None else (k, doc.index(items[k]), at % 16))
        at += len(doc)

    for r in range(16):
        if r:
            add(b"a", None)
        for k, item in enumerate(items):
            for pos in range(bigsigma.EDGE_POSITIONS):
                doc = (filler[:pos] + item + tail)[:112]
                assert len(doc) == 112 and doc[pos:pos + len(item)] == item
                add(doc, k)
        for pos in range(0, bigsigma.EDGE_POSITIONS, 3):      # the truncated rune as the document's last bytes
            doc = (tail[:110 - pos] + filler[:pos]) + items[TRUNCATED]
            assert len(doc) == 112
            add(doc, TRUNCATED)
    return docs, where


def _edge_case():
    """(model image, oracle, docs, text, off, where, the oracle's status per document): made once, shared by the cases
    of test_window_edges and left unchanged."""
    from datok_amd import corpus
    if "edges" not in bigsigma._cache:
        blob = bigsigma.enlarged_de(64, edge=True)
        om = bigsigma.oracle_of(blob)
        docs, where = _edge_documents()
        n_edge = len(docs)
        docs = docs + _backtrack_documents()
        where = where + [None] * (len(docs) - n_edge)
        text, off = corpus.concat_docs(docs)
        status = [om.transduce_doc(doc, 0).status for doc in docs]
        bigsigma._cache["edges"] = (blob, om, docs, text, off, where, status)
    return bigsigma._cache["edges"]


def _backtrack_documents():
    """Tokens of 1..100 bytes followed by text that makes the walk backtrack over blanks and full stops (abbreviations
    that are and are not one, numbers with separators): the window is re-based backwards."""
    l = bigsigma.LETTERS
    tails = [" z. B. 1.000 Euro u. a. m. x", ". z. Bx 1.000.000,5 d. h. nein", bigsigma.STOPS[2] + " Dr. med. h. c. usw. u. v. a. ",
             bigsigma.BLANKS[1] + "i. d. R. 12.345.678 z.B. o. k" + bigsigma.STOPS[0]]
    docs = []
    for n in range(1, 101):
        word = "".join(l[(n + i) % 40] if i % 3 == 0 else "x" for i in range(n))
        word = word.encode("utf-8")[:n].decode("utf-8", "ignore") or "x"
        docs.append((word + tails[n % 4]).encode("utf-8"))
        docs.append(("Am 1.000. Tag z. B. " + word + tails[(n + 1) % 4]).encode("utf-8"))
    return docs


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [0, 16])
def test_window_edges(load, chunk):
    """Every kind of stream entry at every position of a lane's first two rows and one behind them (for rows of up to 32
    entries: bigsigma.EDGE_POSITIONS) and at every alignment of the document in the stream; a truncated rune as a
    document's last bytes; long tokens with backtracking text behind them."""
    import datok_amd
    blob, om, docs, text, off, where, status = _edge_case()
    tok = load("de66.matok", blob)
    # where the items lie, read from the documents: every kind at every position and residue, and which of those
    # documents the oracle gives status 0 (they are compared in full below)
    seen, clean = {}, {}
    for w, s in zip(where, status):
        if w is not None:
            seen.setdefault(w[:2], set()).add(w[2])
            clean.setdefault(w[:2], set()).update([w[2]] if s == 0 else [])
    every = set(range(16))
    for k in range(8):
        for pos in range(bigsigma.EDGE_POSITIONS):
            assert seen.get((k, pos)) == every, (k, pos)
            # an EOT as a document's first rune ends a text without a token (EMPTY_TEXT: the reference panics there);
            # every other document of the set is in contract
            assert clean[(k, pos)] == (set() if (k, pos) == (3, 0) else every), (k, pos)
    assert seen[(TRUNCATED, 110)] == clean[(TRUNCATED, 110)] == every      # ... and as the document's last bytes
    assert all(s in (0, datok_amd.ST_EMPTY_TEXT) for s in status)
    n_clean = sum(1 for s in status if s == 0)
    assert n_clean == len(docs) - 16

    res, tot, out = _run(tok, text, off, chunk=chunk, warm=4, render=3)
    if chunk:
        assert tot["n_lanes"] > len(docs)
    assert tot["n_flagged"] == len(docs) - n_clean
    assert assert_batch_equals_oracle(om, res, text, off) == n_clean
    assert _assert_rendered(om, out, res, docs, 3) == len(docs)      # (SIMPLE prints no positions: EMPTY_TEXT renders too)


@pytest.mark.gpu
def test_batch_ends(load):
    """The last bytes of a batch: one-document batches of 1..40 bytes, a truncated three-byte rune as a batch's last
    bytes, a leading empty document -- on one batch object, each input after a longer one (what lies in the stream
    behind a batch is then the previous run's)."""
    import datok_amd
    from datok_amd import corpus
    blob = bigsigma.enlarged_de(64, edge=True)
    tok, om = load("de66.matok", blob), bigsigma.oracle_of(blob)
    l, s, bl = bigsigma.LETTERS, bigsigma.STOPS, bigsigma.BLANKS
    base = ("Ab" + l[0] + l[7] + bl[0] + "z. B." + bl[3] + l[1] + "x" + s[0] + " 1.000 " + bigsigma.CHAR3 + l[2] + s[1]
            + bigsigma.CHAR4 + " u. a. m").encode("utf-8")
    assert len(base) >= 40
    long_text, long_off, _ = bigsigma.german_spliced()
    cut3 = bigsigma.CHAR3.encode()[:2]
    with datok_amd.Batch(len(long_text), 64) as b:
        def check(docs, chunk):
            text, off = corpus.concat_docs(docs)
            res, tot, out = _run(tok, text, off, chunk=chunk, warm=4, render=3, batch=b)
            assert_batch_equals_oracle(om, res, text, off)
            _assert_rendered(om, out, res, docs, 3)
        for chunk in (None, 0, 16):
            _run(tok, long_text, long_off, batch=b)
            for n in range(1, 41):
                check([base[:n]], chunk)                          # (a cut inside a rune: a truncated rune at the end)
            _run(tok, long_text, long_off, batch=b)
            for n in (0, 1, 7, 8, 9, 15, 16, 17, 30, 31, 32, 33):
                check([b"x" * n + cut3], chunk)
                check([b"Satz eins. ", ("zwei" + l[5]).encode() * 3 + b" " * (n % 5) + cut3], chunk)
            check([b"", base, b"", base[:13] + cut3], chunk)      # a leading empty document
            check([b""], chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,warm", [(None, 64), (64, 0)])
def test_entries_with_64bit_cells(load, chunk, warm):
    """The enlarged model widened to 40 000 states: 64-bit fused cells and 16-bit entries under the lean loop."""
    blob = bigsigma.enlarged_de(64)
    key = ("wide", 40000)
    if key not in bigsigma._cache:
        bigsigma._cache[key] = wide.widen_matok(blob, 40000)
    tok, om = load("de64.wide40000.matok", bigsigma._cache[key]), bigsigma.oracle_of(blob)
    if not _switched():
        assert tok.info["entry_bytes"] == 8 and tok.info["lean_walk"] == 1 and tok.info["state_count"] == 40000, tok.info
    text, off, docs = bigsigma.german_spliced()
    res, tot, out = _run(tok, text, off, chunk=chunk, warm=warm, render=3)
    assert tot["n_flagged"] == 0
    if warm == 0:
        assert tot["repair_rounds"] > 0
    assert assert_batch_equals_oracle(om, res, text, off) == 64
    assert _assert_rendered(om, out, res, docs, 3) == 64


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["datok", "matok"])
def test_double_array_rules_over_entries(load, kind):
    """craft.big_sigma: the dense layout of a double array (its own EOT rules, walk_fused<.., IS_MATRIX = false>) and
    the matrix, over EOT texts."""
    from datok_amd import corpus
    blob, extra = craft.big_sigma(kind)
    tok, om = load("big." + kind, blob), bigsigma.oracle_of(blob)
    assert tok.type() == kind.upper()
    if kind == "datok" and not _switched():
        assert tok.info["dense_states"] > 0
    docs = craft.documents(np.random.default_rng(5))
    rng = np.random.default_rng(6)
    letters = [c.encode() for c in craft.ALPHABET] + [c.encode() for c in extra[:40]]
    for _ in range(200):      # ... and the same kind of text with the new letters in it
        docs.append(b"".join(letters[int(i)] for i in rng.integers(0, len(letters), size=int(rng.integers(0, 80)))))
    text, off = corpus.concat_docs(docs)
    compared = 0
    for chunk, warm in ((0, 0), (16, 4)):
        for flags in (0, NEWLINE_AFTER_EOT):
            res, tot, out = _run(tok, text, off, flags, chunk=chunk, warm=warm, render=3)
            compared += assert_batch_equals_oracle(om, res, text, off, flags)
            _assert_rendered(om, out, res, docs, 3, flags)
    assert compared > 400


@pytest.mark.gpu
@pytest.mark.parametrize("kind,triple", [("datok", False), ("matok", True), ("datok", True)])
def test_exact_pass_over_entries(load, kind, triple):
    """The crafted tokenizers that reach the exact pass (the double array's EOT read twice; three SentenceEnds at one
    cursor) over SIGMA plus 300 characters: the lean loop's policy hands the exact pass its general one.  Call order,
    int arguments and offsets against the oracle."""
    import datok_amd
    from datok_amd import corpus
    from test_exact_and_replay import _oracle_calls, _replayed
    blob, extra = bigsigma.crafted(kind, triple)
    tok, om = load("crafted%d.%s" % (triple, kind), blob), bigsigma.oracle_of(blob)
    docs = craft.documents(np.random.default_rng(5))
    new = extra[3].encode()
    docs += [d.replace(b"a", new, 1) for d in docs[:16]]
    text, off = corpus.concat_docs(docs)
    for chunk, flags in ((0, 0), (16, NEWLINE_AFTER_EOT), (None, 0)):
        with datok_amd.Batch(max(len(text), 1), len(docs)) as b:
            if chunk is not None:
                b.set_chunking(chunk, 8, extend=0)
            b.set_input(text, off)
            b.run(tok, flags)
            res = b.result()
            assert not any(int(s) & datok_amd.ST_IRREGULAR for s in res.status)
            assert assert_batch_equals_oracle(om, res, text, off, flags) > 100
            assert len(res.exact) > 0         # the construct occurred and was handled
            for d, doc in enumerate(docs):
                exp = [c[:3] if c[0] == "T" else c for c in _oracle_calls(om, doc)]
                assert _replayed(res, d, doc, kind == "matok") == exp, (d, doc)


@pytest.mark.gpu
def test_one_long_document(load):
    """300 KB in one document: more than 64 lanes, compacted in segments."""
    blob = bigsigma.enlarged_de(64)
    tok, om = load("de64.matok", blob), bigsigma.oracle_of(blob)
    text, _, _ = bigsigma.german_spliced(80, 4096, seed=33)
    text = text[:300_000]
    while text[-1] & 0xC0 == 0x80 or text[-1] >= 0xC0:      # (not inside a rune)
        text = text[:-1]
    off = np.array([0, len(text)], dtype=np.uint64)
    res, tot, out = _run(tok, text, off, render=3)
    assert tot["n_lanes"] > 64 and tot["n_flagged"] == 0
    assert assert_batch_equals_oracle(om, res, text, off) == 1
    assert out[0] == om.transduce(text.tobytes(), 3)[0]


_OLD_PATH_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import datok_amd
tok = datok_amd.load_tokenizer_file(sys.argv[2])
assert tok is not None and tok.info["stream_codes"] == 0 and tok.info["lean_walk"] == int(sys.argv[5]), tok.info
z = np.load(sys.argv[3])
text, off = z["text"], z["off"]
with datok_amd.Batch(len(text), len(off) - 1) as b:
    b.set_input(text, off); b.run(tok, 0)
    res = b.result()
    np.savez(sys.argv[4], **{f: np.asarray(getattr(res, f)) for f in sys.argv[6].split(",")})
print("CHILD OK")
"""
_ARRAYS = ("tok_off", "sent_off", "text_off", "tok_rstart", "tok_rend", "tok_bstart", "tok_bend", "sent", "text_tok_end",
           "text_sent_end", "status", "ev_bits", "doc_tail")


@pytest.mark.gpu
def test_against_the_general_loop(load, tmp_path):
    """DATOK_GENERAL16=1 keeps a model of 16-bit entries on the general loop, the path it took before: the same batch,
    array by array (event bitmaps included)."""
    if _switched():
        pytest.skip("already running under a switch that selects a table encoding or a loop")
    blob = bigsigma.enlarged_de(64)
    tok = load("de64.matok", blob)
    text, off, docs = bigsigma.german_spliced()
    script, img, inp, outp = tmp_path / "child.py", tmp_path / "de64.matok", tmp_path / "in.npz", tmp_path / "out.npz"
    script.write_text(_OLD_PATH_SCRIPT)
    img.write_bytes(blob)
    np.savez(inp, text=text, off=off)
    e = dict(os.environ)
    e["DATOK_GENERAL16"] = "1"
    r = subprocess.run([sys.executable, str(script), ROOT, str(img), str(inp), str(outp), "0", ",".join(_ARRAYS)],
                       capture_output=True, env=e, timeout=300)
    assert r.returncode == 0 and b"CHILD OK" in r.stdout, r.stderr.decode()[-2000:]
    res, tot, _ = _run(tok, text, off)
    old = np.load(outp)
    assert len(old["tok_rstart"]) == tot["n_tokens"] > 64 * 400
    for f in _ARRAYS:
        assert np.array_equal(np.asarray(getattr(res, f)), old[f]), f


@pytest.mark.gpu
def test_existing_suite_over_entries():
    """DATOK_SYM16=1 gives every shipped model a stream of 16-bit entries, and with it the new loop: the goldens through
    the C-ABI and the Python token writer, and the speculative-chunk tests (three models, warm-ups 0 and 4 among them),
    in a process of their own.  20 tests; measured on an MI355X machine: 5.1 s for the child (this whole file: 8.9 s)."""
    if _switched() or os.environ.get("DATOK_SYM16"):
        pytest.skip("already running under a switch that selects a table encoding, a stream format or a loop")
    e = dict(os.environ)
    e["DATOK_SYM16"] = "1"
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "goldens_through or speculative_chunks", os.path.join(ROOT, "tests", "test_gpu_parity.py")],
                       capture_output=True, env=e, timeout=240, cwd=ROOT)
    print("child suite: %.1f s" % (time.time() - t0))
    assert r.returncode == 0, (r.stdout.decode()[-1500:], r.stderr.decode()[-500:])
    assert b"20 passed" in r.stdout, r.stdout.decode()[-300:]
