"""A closure replay's sparse events as a list (DTK_R_EVENT_LIST, include/datok_gpu.h): evl_off / evl_pos / evl_kind in
place of the five event bitmaps -- about one 5-byte entry per sentence instead of five bits per input byte.

CPU tier: the replays (datok_amd.replay_list, detail::replay_list of include/datok.hpp) driven by lists made from the
oracle's calls (tests/evlist.py), and their bytes against the oracle's own writer.
GPU tier: the kernels of dtk_evlist.hip and the download path -- the delivered list equals, entry for entry, the numpy
definition of tests/evlist.py applied to the bitmaps of the same run, and the replay from it logs the oracle's calls.
"""
import gzip
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import blocked
import craft
import evlist
from conftest import MODELS, ROOT
from test_host_logic import TEXTS, matrix_events

NEWLINE_AFTER_EOT, OFFSETS_ONLY, NO_RUNE_OFFSETS = 16, 256, 1024
MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")
WRITER_FLAGS = (3, 7, 12, 28, 31)


# ---------------------------------------------------------------------------------------------------- CPU tier
_lists = {}


def _oracle_lists(om):
    """Per document of TEXTS + five_documents(): (bytes, evl_pos, evl_kind, tail, tok_bstart, tok_bend) made from the
    oracle's calls by matrix_events -> evlist.from_event_bytes.  Computed once and shared (read only)."""
    if not _lists:
        rows = []
        for raw in [t.encode() for t in TEXTS] + blocked.five_documents():
            if om.transduce(raw, 3)[1]:
                continue
            ev, starts = matrix_events(om, raw)
            pos, kind, tail, ends = evlist.from_event_bytes(ev)
            exp = om.transduce_doc(raw, 0)
            # the k-th END bit of a document is at cursor tok_bend[k]; n_sent + n_texts bounds the entries
            assert np.array_equal(ends, exp.tok_bend) and np.array_equal(starts, exp.tok_bstart), raw[:40]
            assert len(pos) <= len(exp.sent) + len(exp.text_tok_end), raw[:40]
            rows.append((raw, pos, kind, tail, starts, ends))
        _lists["rows"] = rows
    return _lists["rows"]


@pytest.mark.parametrize("flags", WRITER_FLAGS)
def test_python_replay_list_prints_the_oracles_bytes(oracle_models, flags):
    """host.replay_list on lists made from the oracle's calls, into new_token_writer: the oracle's bytes."""
    import datok_amd
    om = oracle_models(MODELS_DE[0])
    rows = _oracle_lists(om)
    assert len(rows) >= len(TEXTS) + 4 and sum(len(r[1]) for r in rows[-5:]) > 3000
    for raw, pos, kind, tail, starts, ends in rows:
        w = io.BytesIO()
        tw = datok_amd.new_token_writer(w, flags)
        datok_amd.replay_list(True, raw, pos, kind, tail, starts, ends, tw)
        tw.Flush()
        assert w.getvalue() == om.transduce(raw, flags)[0], (raw[:40], flags)


def test_python_replay_list_logs_the_oracles_calls(oracle_models):
    """The int arguments too: the recording writer of tests/evlist.py against oracle.Model.events()."""
    import datok_amd
    om = oracle_models(MODELS_DE[0])
    for raw, pos, kind, tail, starts, ends in _oracle_lists(om):
        rec = evlist.Recorder()
        datok_amd.replay_list(True, raw, pos, kind, tail, starts, ends, rec)
        assert rec.calls == evlist.oracle_calls(om, raw), raw[:40]


_CPP = r'''
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>
#include "datok.hpp"
// argv: view file, "wide" | "blk", writer flags.  The file: u32 n_docs, u32 n_tok, u32 n_evl, u32 text bytes, then
// doc_off u64[n_docs + 1], tok_off u64[n_docs + 1], text, tok_bstart, tok_bend, words u32[n_tok], heads 16 B per
// block, evl_off u32[n_docs + 1], evl_pos u32[n_evl], doc_tail u32[n_docs], evl_kind u8[n_evl].
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<unsigned char> raw;
  unsigned char chunk[4096];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) raw.insert(raw.end(), chunk, chunk + got);
  fclose(f);
  uint32_t h[4];
  memcpy(h, raw.data(), 16);
  const uint32_t nd = h[0], nt = h[1], ne = h[2], nb = h[3];
  const unsigned char *q = raw.data() + 16;
  auto take = [&](size_t bytes) { const unsigned char *p = q; q += (bytes + 7) & ~(size_t)7; return p; };
  const uint64_t *doc_off = (const uint64_t *)take(8 * (nd + 1));
  dtk_result_view v;
  memset(&v, 0, sizeof v);
  v.tok_off = (const uint64_t *)take(8 * (nd + 1));
  const uint8_t *text = take(nb);
  const uint32_t *bstart = (const uint32_t *)take(4 * nt), *bend = (const uint32_t *)take(4 * nt);
  const uint32_t *words = (const uint32_t *)take(4 * nt);
  const dtk_off_block *heads = (const dtk_off_block *)take(16 * ((nt + 63) / 64));
  v.evl_off = (const uint32_t *)take(4 * (nd + 1));
  v.evl_pos = (const uint32_t *)take(4 * ne);
  v.doc_tail = (const uint32_t *)take(4 * nd);
  v.evl_kind = take(ne);
  if (q > raw.data() + raw.size()) return 4;
  if (!strcmp(argv[2], "blk")) { v.tok_bblk = words; v.tok_bblk_head = heads; }   // (only the blocked form was delivered)
  else { v.tok_bstart = bstart; v.tok_bend = bend; }
  std::ostringstream os;
  for (uint32_t d = 0; d < nd; d++) {
    auto tw = datok::NewTokenWriter(os, (datok::Bits)atoi(argv[3]));
    datok::detail::replay_list(true, text + doc_off[d], (size_t)(doc_off[d + 1] - doc_off[d]), v, d, *tw);
    tw->Flush();
  }
  std::cout << os.str();
  return 0;
}
'''


def test_cpp_replay_list_prints_the_oracles_bytes(oracle_models, tmp_path):
    """detail::replay_list of include/datok.hpp in a stand-alone host program, on a hand-built view of several
    documents read from a file: once with the 32-bit byte offsets, once with their blocked form only."""
    om = oracle_models(MODELS_DE[0])
    rows = [r for r in _oracle_lists(om) if len(r[0]) < 80000]    # TEXTS, "Ein Baum." and the tokens of 1000 bytes
    assert len(rows) >= len(TEXTS) - 1 and sum(len(r[4]) for r in rows) > 64     # (more than one block of 64 tokens)
    docs = [r[0] for r in rows]
    doc_off = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.uint64)
    tok_off = np.concatenate([[0], np.cumsum([len(r[4]) for r in rows])]).astype(np.uint64)
    evl_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.uint32)
    bstart, bend = (np.concatenate([r[k] for r in rows]).astype(np.uint32) for k in (4, 5))
    words, heads, overflow, _ = blocked.encode(bstart, bend)
    assert overflow == 0
    pos, kind = np.concatenate([r[1] for r in rows]).astype(np.uint32), np.concatenate([r[2] for r in rows]).astype(np.uint8)
    tails = np.array([r[3] for r in rows], dtype=np.uint32)
    text = b"".join(docs)

    def pad(b):
        return b + b"\0" * (-len(b) % 8)
    blob = struct.pack("<4I", len(docs), len(bstart), len(pos), len(text)) + b"".join(
        pad(a if isinstance(a, bytes) else a.tobytes())
        for a in (doc_off, tok_off, text, bstart, bend, words, heads, evl_off, pos, tails, kind))
    src, exe, view = tmp_path / "rl.cpp", tmp_path / "rl", tmp_path / "view.bin"
    src.write_text(_CPP)
    view.write_bytes(blob)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    for flags in WRITER_FLAGS:
        exp = b"".join(om.transduce(x, flags)[0] for x in docs)
        for form in ("wide", "blk"):
            assert subprocess.check_output([str(exe), str(view), form, str(flags)]) == exp, (form, flags)


def test_numpy_definition_on_hand_made_bitmaps():
    """tests/evlist.py itself on three documents of 3, 0 and 30 bytes: cursor 0 and cursor len, a word boundary, a
    document without entries, kinds that share a cursor, and a stray bit behind the batch's end."""
    doc_off = np.array([0, 3, 3, 33], dtype=np.uint64)
    bits = np.zeros((5, 4), dtype=np.uint32)

    def put(kind, g):
        bits[kind, g >> 5] |= np.uint32(1 << (g & 31))
    put(evlist.EVB_SEPS, 0); put(evlist.EVB_SEPS, 3)                 # document 0: cursors 0 and 3 = len
    put(evlist.EVB_SEOT, 5 + 26); put(evlist.EVB_TEOT, 5 + 26)       # document 2 starts at bit 5: global bits 31 and 32
    put(evlist.EVB_SEPS, 5 + 27); put(evlist.EVB_TEOT, 5 + 30)       # ... and its cursor len
    put(evlist.EVB_SEPS, 36); put(0, 7); put(1, 9)                   # behind the end; END and START are not listed
    off, pos, kind, g = evlist.from_bitmaps(bits, doc_off)
    assert off.tolist() == [0, 2, 2, 5] and off.dtype == np.uint32 and pos.dtype == np.uint32 and kind.dtype == np.uint8
    assert pos.tolist() == [0, 3, 26, 27, 30] and kind.tolist() == [4, 4, 3, 4, 2] and g.tolist() == [0, 3, 31, 32, 35]


# ---------------------------------------------------------------------------------------------------- GPU tier
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


def _replay_fields():
    B = _B()
    return B.R_EVENT_LIST | B.R_EVENTS | B.R_TOK_BYTE | B.R_CSR | B.R_STATUS


def _assert_list_equals_bitmaps(r, off):
    """The delivered list against tests/evlist.py on the delivered bitmaps: entry for entry, dtypes included."""
    e_off, e_pos, e_kind, g = evlist.from_bitmaps(r.ev_bits, off)
    for name, exp in (("evl_off", e_off), ("evl_pos", e_pos), ("evl_kind", e_kind)):
        got = getattr(r, name)
        assert got.dtype == exp.dtype and got.shape == exp.shape, (name, got.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (name, np.flatnonzero(got != exp)[:4])
    assert len(r.doc_tail) == len(off) - 1 and (len(e_kind) == 0 or int(r.evl_kind.min()) > 0)
    return g


def _assert_replays_equal_oracle(r, docs, om, is_matrix, ids=None):
    n = 0
    for d in (range(len(docs)) if ids is None else ids):
        if om.transduce_doc(docs[d], 0).status & 1:      # (window overflow: the reference dies there)
            continue
        assert evlist.replayed(r, d, docs[d], is_matrix) == evlist.oracle_calls(om, docs[d]), (d, docs[d][:60])
        n += 1
    return n


def _run(tok, docs, fields, flags=0, batch=None):
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    b = batch or _B()(max(len(text), 1), len(docs))
    try:
        b.set_input(text, off)
        b.set_result_fields(fields)
        b.run(tok, flags)
        return b.result(), off, b.totals()
    finally:
        if batch is None:
            b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, NEWLINE_AFTER_EOT])
@pytest.mark.parametrize("model", MODELS_DE)
def test_list_against_bitmaps_and_oracle(gpu, oracle_models, model, flags):
    """five_documents(): the list equals the numpy definition on the delivered bitmaps, and the recording writer fed by
    replay_list logs the oracle's calls, int arguments included, for every document."""
    docs = blocked.five_documents()
    r, off, tot = _run(gpu(model), docs, _replay_fields(), flags)
    _assert_list_equals_bitmaps(r, off)
    assert 3000 < len(r.evl_pos) <= tot["n_sent"] + tot["n_texts"] and not r.status.any() and not r.exact
    assert _assert_replays_equal_oracle(r, docs, oracle_models(model), model.endswith(".matok")) == 5


def _edge_documents():
    docs = [b""] * 9                                                            # a run of empty documents at the head
    docs += [(b"Ja. Nein! " * 20)[:L] for L in range(161)]
    docs += [b"", b"a", b"\x04", "Tree\n\x04\n".encode(), "This.\n\x04And.\n\x04\n".encode()]
    docs += [b""] * 33                                                          # ... in the middle
    docs += [b"   ", b"und so weiter ohne Ende", b"\n"]
    docs += [("Gut.\n\x04\nEnde? Grüße! " * 9)[:L].encode() for L in range(161)]
    docs += [b""] * 21                                                          # ... and at the end
    return docs


def _check_edges(r, off, docs, om, is_matrix):
    g = _assert_list_equals_bitmaps(r, off)
    assert _assert_replays_equal_oracle(r, docs, om, is_matrix) == len(docs)
    lens = np.diff(off.astype(np.int64))
    per_doc = np.diff(r.evl_off.astype(np.int64))
    d_of = np.repeat(np.arange(len(docs)), per_doc)
    print("edges: %d entries, %d at cursor 0, %d at cursor len, %d documents without, word bits 31/0: %d/%d" % (
        len(g), int((r.evl_pos == 0).sum()), int((r.evl_pos == lens[d_of]).sum()), int((per_doc == 0).sum()),
        int((g % 32 == 31).sum()), int((g % 32 == 0).sum())))
    assert int(r.evl_off[-1]) == len(r.evl_pos) == len(g) and int(r.evl_off[0]) == 0
    assert (r.evl_pos == lens[d_of]).any()                                      # cursor len (cursor 0: see below)
    # a document of one byte with an entry at its len, the next document's cursor 0 on the next bit: the lone EOT.
    # ("a" has none: its final SentenceEnd is no epsilon call but the S bit of its tail word, like the empty document's)
    a, e = docs.index(b"a"), docs.index(b"\x04")
    assert per_doc[a] == 0 and int(r.doc_tail[a]) == (1 << 2 | 3)
    assert per_doc[e] == 1 and int(r.evl_pos[int(r.evl_off[e])]) == 1 and int(r.evl_kind[int(r.evl_off[e])]) == 3
    assert (g % 32 == 31).any() and (g % 32 == 0).any()                         # both sides of a word boundary
    assert (per_doc == 0).any() and (per_doc > 1).any()                         # documents without entries


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS_DE)
def test_edges(gpu, oracle_models, model):
    """About 400 documents: every length 0..160 of two texts, the empty document, "a", a lone EOT, texts that end in
    an EOT, runs of empty documents at the head, in the middle and at the end of the batch."""
    docs = _edge_documents()
    assert 380 <= len(docs) <= 420
    r, off, _ = _run(gpu(model), docs, _replay_fields())
    _check_edges(r, off, docs, oracle_models(model), model.endswith(".matok"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["matok", "datok"])
def test_entry_at_cursor_zero(tmp_path, kind):
    """No document of test_edges has an entry at cursor 0 with the shipped tokenizers: their start state has no
    epsilon arc, and the SentenceEnd of an empty document is a bit of its tail word.  A hand-made tokenizer whose start
    state has one fires SentenceEnd in front of the first token of "b": an entry at cursor 0, also in the first
    document of the batch (global bit 0) and right behind a run of empty documents."""
    from craft import A, B, DOT, E, EPS, NL, SP
    arcs = {1: {EPS: (2, False), A: (3, False)},
            2: {A: (3, False), B: (3, False), DOT: (3, False), SP: (2, True), NL: (2, True), E: (2, True)},
            3: {A: (3, False), B: (3, False), EPS: (2, False)}}
    docs = [b"b", b"", b"", b"b b", b"a", b" b", b"ab. b\x04b", b"", b"b" * 40, b"a b " * 30, b"b"]
    import datok_amd
    from oracle import oracle as O
    blob = getattr(craft, kind + "_from")(arcs)
    path = tmp_path / ("eps0." + kind)
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), O.Model(raw=gzip.decompress(blob))
    assert evlist.oracle_calls(om, b"b")[:2] == [("S", 0), ("T", 0, 1)]
    r, off, _ = _run(tok, docs, _replay_fields())
    g = _assert_list_equals_bitmaps(r, off)
    assert _assert_replays_equal_oracle(r, docs, om, kind == "matok") == len(docs)
    zero = np.flatnonzero(r.evl_pos == 0)
    assert len(zero) >= 4 and int(g[0]) == 0 and int(r.evl_kind[0]) == 4
    assert int(r.evl_off[3]) in zero and int(r.evl_off[len(docs) - 1]) in zero


@pytest.mark.gpu
def test_tiles(gpu, oracle_models):
    """3 000 documents of lengths (37 i) mod 257: 380 KB + 3 000 cursor positions are twelve tiles of 32 768 bits, the
    last one ragged.  The list equals the numpy definition; 50 sampled documents replay to the oracle's calls."""
    from datok_amd import corpus
    t, _ = corpus.german_docs(1, 400000, seed=43)
    raw = t.tobytes()
    lens = [(37 * i) % 257 for i in range(3000)]
    cuts = np.concatenate([[0], np.cumsum(lens)])
    docs = [raw[int(cuts[i]):int(cuts[i + 1])] for i in range(3000)]
    n_bits = int(cuts[-1]) + 3000
    assert n_bits // 32768 >= 3 and n_bits % 32768 not in (0, 32767) and 370000 < cuts[-1] < 400000
    model = MODELS_DE[0]
    r, off, tot = _run(gpu(model), docs, _replay_fields())
    g = _assert_list_equals_bitmaps(r, off)
    assert len(np.unique(g // 32768)) >= 3 and len(g) > 1000
    ids = np.random.default_rng(6).choice(3000, size=50, replace=False).tolist()
    assert _assert_replays_equal_oracle(r, docs, oracle_models(model), True, ids) == 50


@pytest.mark.gpu
def test_short_fall_and_reuse(gpu, oracle_models):
    """EVL_CAP=1: the copies are sized for one entry, dtk_batch_result_host sees the count, grows, packs and copies
    again -- the result is complete.  Then one batch object small -> five_documents() -> small: no stale entry, no
    stale offset of the larger run."""
    import datok_amd
    model = MODELS_DE[0]
    tok, om = gpu(model), oracle_models(model)
    docs = _edge_documents()
    assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"1") == 0
    try:
        from datok_amd import corpus
        text, off = corpus.concat_docs(docs)
        with _B()(len(text), len(docs)) as b:
            b.set_input(text, off)
            b.set_result_fields(_replay_fields())
            b.run(tok, 0)
            for _ in range(2):                      # (a second call neither copies again nor loses the list)
                r = b.result()
                _check_edges(r, off, docs, om, True)
            b.run(tok, OFFSETS_ONLY | NO_RUNE_OFFSETS)     # the next run falls short again, with an offsets-only flag
            r = b.result()
            _check_edges(r, off, docs, om, True)
    finally:
        assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"-1") == 0
    small = [b"Ein Baum. Zwei!", b"", "Tree\n\x04\n".encode()]
    five = blocked.five_documents()
    with _B()(sum(len(x) for x in five), 8) as b:
        first = None
        for k, batch_docs in enumerate((small, five, small)):
            r, off, tot = _run(tok, batch_docs, _replay_fields(), batch=b)
            _assert_list_equals_bitmaps(r, off)
            assert len(r.evl_pos) <= tot["n_sent"] + tot["n_texts"]
            assert _assert_replays_equal_oracle(r, batch_docs, om, True) == len(batch_docs)
            if k == 0:
                first = r
        for name in ("evl_off", "evl_pos", "evl_kind", "doc_tail"):
            assert np.array_equal(getattr(r, name), getattr(first, name)), name
        assert len(r.evl_off) == 4 and 0 < len(r.evl_pos) < 10


@pytest.mark.gpu
def test_selection(gpu, oracle_models):
    """R_EVENT_LIST | R_TOK_BYTE_BLK | R_CSR | R_STATUS -- the narrowest download of a closure replay: no bitmaps, the
    tail words and the list are there, and the replay from the blocked byte offsets equals the oracle.  R_EVENTS alone
    and the device view leave the three pointers NULL; an unknown bit is still DTK_E_ARG."""
    import ctypes as C
    import datok_amd
    from datok_amd import _lib, corpus
    B = _B()
    model = MODELS_DE[1]
    docs = blocked.five_documents()[1:] + _edge_documents()[150:200]
    text, off = corpus.concat_docs(docs)
    with B(len(text), len(docs)) as b:
        b.set_input(text, off)
        b.set_result_fields(B.R_EVENT_LIST | B.R_TOK_BYTE_BLK | B.R_CSR | B.R_STATUS)
        b.run(gpu(model), 0)
        r = b.result()
        assert r.ev_bits.shape == (5, 0) and len(r.tok_bstart) == 0 and len(r.tok_bend) == 0
        assert len(r.doc_tail) == len(docs) and len(r.evl_off) == len(docs) + 1 and len(r.tok_bblk) == b.totals()["n_tokens"]
        assert len(r.evl_pos) == len(r.evl_kind) == int(r.evl_off[-1]) > 2000
        assert _assert_replays_equal_oracle(r, docs, oracle_models(model), False) == len(docs)
        v = _lib.ResultView()
        _lib.check(datok_amd.lib().dtk_batch_result_host(b._h, C.byref(v)))
        assert v.evl_off and v.evl_pos and v.evl_kind and v.doc_tail and not v.ev_bits
        b.set_result_fields(B.R_EVENTS)
        b.run(gpu(model), 0)
        _lib.check(datok_amd.lib().dtk_batch_result_host(b._h, C.byref(v)))
        assert v.ev_bits and v.doc_tail and not (v.evl_off or v.evl_pos or v.evl_kind)
        v = b.result_device()
        assert v.ev_bits and v.doc_tail and not (v.evl_off or v.evl_pos or v.evl_kind)
        with pytest.raises(_lib.DatokGpuError) as e:
            b.set_result_fields(B.R_EVENT_LIST | 4096)
        assert e.value.code == _lib.E_ARG
        b.set_result_fields(B.R_EVENT_LIST)            # (the list alone: doc_tail comes with it)
        r = b.result()
        assert len(r.doc_tail) == len(docs) and len(r.evl_pos) > 2000 and r.ev_bits.shape[1] > 0   # (R_EVENTS came before)


def _pipeline_documents():
    from datok_amd import corpus
    t, o = corpus.german_docs(64, 6144, seed=47)
    docs = [t[int(o[d]):int(o[d + 1])].tobytes()[:2048 + 64 * d].rsplit(b" ", 1)[0] for d in range(64)]
    docs[7] += b"\n\x04\nUnd noch ein Text."
    return docs


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [False, True])
def test_pipeline(gpu, oracle_models, multi):
    """64 documents of 2-6 KB in slices of 32 KB, depth 3, the field set on the pipeline: every document of every
    slice replays to the oracle's calls.  Once through dtk_pipeline, once through dtk_multi with the device listed once."""
    import datok_amd
    from datok_amd import corpus
    B = _B()
    model = MODELS_DE[0]
    om = oracle_models(model)
    docs = _pipeline_documents()
    assert min(map(len, docs)) >= 2000 and max(map(len, docs)) <= 6200
    text, off = corpus.concat_docs(docs)
    seen = []

    def on_slice(first, n, b):
        r = b.result(copy=False)
        assert len(r.evl_off) == n + 1 and len(r.doc_tail) == n and r.ev_bits.shape[1] == 0 and len(r.tok_bblk) == b.totals()["n_tokens"]
        assert _assert_replays_equal_oracle(r, docs[first:first + n], om, True) == n
        seen.append(n)
    fields = B.R_EVENT_LIST | B.R_TOK_BYTE_BLK | B.R_CSR | B.R_STATUS
    if multi:
        with datok_amd.MultiPipeline(os.path.join(MODELS, model), [0], 32 << 10, 64, depth=3) as p:
            p.set_result_fields(fields)
            p.run(text, off, 0, on_slice)
    else:
        with datok_amd.Pipeline(32 << 10, 64, depth=3) as p:
            p.set_result_fields(fields)
            p.run(gpu(model), text, off, 0, on_slice)
    assert sum(seen) == len(docs) and len(seen) >= 6


def _crafted_check(tmp_path, name, blob, docs, want_exact):
    import datok_amd
    from oracle import oracle as O
    path = tmp_path / name
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), O.Model(raw=gzip.decompress(blob))
    assert tok is not None
    r, off, _ = _run(tok, docs, _replay_fields())
    _assert_list_equals_bitmaps(r, off)
    assert not any(int(s) & datok_amd.ST_IRREGULAR for s in r.status)
    assert _assert_replays_equal_oracle(r, docs, om, tok.type() == "MATOK") > len(docs) // 2
    if want_exact:
        assert 0 < len(r.exact) < len(docs)      # some documents replay from `calls`, all others from the list
    return len(r.exact)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["matok", "datok"])
def test_exact_pass_documents_replay_from_calls(tmp_path, kind):
    """A crafted tokenizer of tests/craft.py (an EOT consumed twice, three epsilon SentenceEnds at one cursor): the
    documents in exact_doc replay from `calls`, all others from the list, and all equal the oracle."""
    docs = craft.documents(np.random.default_rng(5))
    _crafted_check(tmp_path, "crafted." + kind, getattr(craft, kind)(True), docs, True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 9, 14])
def test_random_automata(tmp_path, seed):
    """craft.random_automaton in both file formats on craft.random_documents: the same check.  (Seeds of
    test_exact_and_replay.py's FUZZ_SEEDS whose matrix image ends no document the way the next test describes.)"""
    rng = np.random.default_rng(seed)
    arcs = craft.random_automaton(rng)
    docs = craft.random_documents(rng)
    for kind in ("matok", "datok"):
        _crafted_check(tmp_path, "fuzz." + kind, getattr(craft, kind + "_from")(arcs), docs, False)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 63])
def test_random_automata_whose_last_token_ends_in_the_eof_branch(tmp_path, seed):
    """Seed 3 sends no document to the exact pass (every one replays from the list), seed 63 a quarter.  Their matrix
    images do what no shipped or crafted tokenizer does: the last token of a document is flushed by the EOF branch
    itself (matrix.go:677), which does not rewind the window, so the final SentenceEnd / TextEnd (matrix.go:683-691)
    pass the length of that token's buffer where they pass 0 behind a token flushed by an epsilon arc.  Bitmaps and
    tail word look the same in both cases, so the bitmap replay passes 0 (121 of seed 3's 172 documents and 6 of seed
    63's differ from the oracle in these ints and in nothing else, measured with host.replay on the bitmaps).  The list
    is a pure function of the bitmaps and replay_list keeps replay's rules: here the list replay must log exactly
    what the bitmap replay logs, the oracle's calls in order with the oracle's Token arguments, and for the double
    array (datok.go:1119,1127 pass 0) the oracle's calls in full."""
    import datok_amd
    from datok_amd import host
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    arcs = craft.random_automaton(rng)
    docs = craft.random_documents(rng)

    def strip(calls):
        return [c if c[0] == "T" else c[:1] for c in calls]
    for kind in ("matok", "datok"):
        blob = getattr(craft, kind + "_from")(arcs)
        path = tmp_path / ("fuzz." + kind)
        path.write_bytes(blob)
        tok, om = datok_amd.load_tokenizer_file(str(path)), O.Model(raw=gzip.decompress(blob))
        r, off, _ = _run(tok, docs, _replay_fields())
        _assert_list_equals_bitmaps(r, off)
        from_list = 0
        for d, doc in enumerate(docs):
            if om.transduce_doc(doc, 0).status & 1:
                continue
            got, exp = evlist.replayed(r, d, doc, kind == "matok"), evlist.oracle_calls(om, doc)
            if d not in r.exact:
                rec = evlist.Recorder()
                a, b = int(r.tok_off[d]), int(r.tok_off[d + 1])
                host.replay(kind == "matok", doc, r.events(d), r.tok_bstart[a:b], rec)
                assert got == rec.calls, (kind, d, doc[:60])
                from_list += 1
            assert strip(got) == strip(exp), (kind, d, doc[:60])
            if kind == "datok":
                assert got == exp, (d, doc[:60])
        assert from_list > 80
