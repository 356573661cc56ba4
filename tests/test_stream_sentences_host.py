"""A stream's sentence rows without a GPU: streamsens.sentences_slice_ref -- the rows one slice's calls close, from the
row carried in -- on synthetic slice views cut from the oracle's calls.  The slices' rows joined are the table of the
whole stream as one document (sentences.from_calls + sentences.rows_of on the oracle's calls and rune offsets), and the
inputs contain rows that span a cut with tokens on both sides and carried rows that the next slice closes without a
token of its own.  Then the C-ABI's two calls and their structs."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import streamcorpus as sc
from streamoffs import offsets_slice_ref
from streampos import CARRY0
from streamsens import SEN_CARRY0, SIX, assert_table, join_sentences, sentences_slice_ref, stream_table
from test_stream_positions_host import empty_text_streams

MODELS = ["tokenizer_de.matok", "tokenizer_de.datok"]
NL = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_DIR = os.path.join(ROOT, "tests", "golden", "models")


def _check(om, raw, empty_text=False, only=SIX):
    """Runs the reference over the synthetic slices of `raw`, compares the joined rows with the whole stream's table and
    returns what kinds of cross-cut rows it met, per run."""
    is_matrix = om.type() == "MATOK"
    calls, st = sc.oracle_calls(om, raw)
    assert st == (sc.ST_EMPTY_TEXT if empty_text else 0) or raw.count(b"a" * 5000)
    slices = sc.synthetic_slices(is_matrix, raw, calls, sc.S)
    assert len(slices) >= 2
    kinds = collections.Counter()
    for nl in (0, NL):
        carry, sen, parts = CARRY0, SEN_CARRY0, []
        for i, sl in enumerate(slices):
            o = offsets_slice_ref(is_matrix, sl, nl, carry)
            r = sentences_slice_ref(is_matrix, sl, nl, carry, sen)
            assert len(r[0]) == len(r[1]) == len(r[2]) == len(r[3]) == len(r[4]) and len(r[5]) == len(o[3]), (nl, i)
            assert r[6][0] == (not o[5][1] and not sl.last), (nl, i)          # open == !sentB of the writer's carry
            if sen[0] and len(r[0]):
                kinds["spans" if r[0][0] > 0 else "closed_without_token"] += 1
                assert (r[1][0], r[3][0]) == (sen[1], sen[3]), (nl, i)           # the carried row keeps its start
                if r[0][0] == 0:
                    assert (r[2][0], r[4][0]) == (sen[2], sen[4]), (nl, i)       # ... and here its end
            parts.append((len(sl.tok_bend),) + r[:6])
            carry, sen = o[5], r[6]
        assert sen == SEN_CARRY0                                                 # the end of the calls closes the last row
        doc = om.transduce_doc(raw, nl)
        assert_table(join_sentences(parts), stream_table(calls, doc), (nl,), only)
    return kinds


@pytest.mark.parametrize("model", MODELS)
def test_reference_joins_to_the_streams_table_on_the_200k_stream(oracle_models, model):
    om = oracle_models(model)
    raw = sc.running_text(200 * 1024, seed=5)
    assert raw.count(b"\x04") >= 10
    kinds = _check(om, raw)
    assert kinds["spans"] >= 2, kinds            # rows that take tokens on both sides of a cut, in both runs


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("construct", list(sc.CONSTRUCTS))
def test_reference_joins_at_every_cut_alignment(oracle_models, model, construct):
    om = oracle_models(model)
    kinds = collections.Counter()
    for shift in (0, 1, 2, 3, 39):
        # (the reference ends at a token that fits no window, the synthetic slices go on: the token ranges still agree)
        kinds += _check(om, sc.construct_stream(construct, shift), only=("sen_tok_end",) if construct == "token5000" else SIX)
    if construct in ("eot_before", "eot_at"):
        assert kinds["closed_without_token"] >= 1, kinds   # the SEOT / TEOT kept at the cut is the next slice's first call


@pytest.mark.parametrize("model", MODELS)
def test_reference_follows_empty_texts(oracle_models, model):
    om = oracle_models(model)
    kinds = collections.Counter()
    for raw, empty in empty_text_streams():
        kinds += _check(om, raw, empty_text=empty)
    assert kinds["closed_without_token"] >= 1, kinds


def test_the_single_text_of_five_slices(oracle_models):
    om = oracle_models("tokenizer_de.matok")
    raw = sc.running_text(5 * sc.S, seed=21).replace(b"\x04", b" ")
    kinds = _check(om, raw)
    assert kinds["spans"] + kinds["closed_without_token"] >= 1, kinds


def test_a_carried_row_closed_in_front_of_any_token():
    """One slice by hand (test_stream_offsets_host.py's): the SEOT of the text that began earlier fires before any token
    of this slice and closes the carried row, which gets no token here."""
    from datok_amd import host
    text = b"x.\x04\nab c"
    sl = host.SliceView(base=16384, first=2, cut=len(text), last=1, status=0, text=text,
                        tok_bstart=np.array([4, 7], np.uint32), tok_bend=np.array([6, 8], np.uint32),
                        evl_pos=np.array([3], np.uint32), evl_kind=np.array([host.EVL_SEOT | host.EVL_TEOT], np.uint8),
                        tail=len(text) << 2 | 3)
    carry = (7, False, False, True, True)
    sen = (True, 16000, 16385, 2, 7)
    r = sentences_slice_ref(True, sl, 0, carry, sen)
    rows = list(zip(*(x.tolist() for x in r[:5])))
    assert rows == [(0, 16000, 16385, 2, 7), (2, 16384 + 4, 16384 + 8, 1, 5)]
    assert r[5].tolist() == [1, 2] and r[6] == SEN_CARRY0
    r = sentences_slice_ref(True, sl, NL, carry, sen)                    # the newline rule moves the rune spans
    assert list(zip(*(x.tolist() for x in r[:5])))[1] == (2, 16384 + 4, 16384 + 8, 0, 4)
    sl.last, sl.tail = 0, 0                                              # without the tail the second row stays open
    r = sentences_slice_ref(True, sl, 0, carry, sen)
    assert list(zip(*(x.tolist() for x in r[:5]))) == [(0, 16000, 16385, 2, 7)]
    assert r[5].tolist() == [1] and r[6] == (True, 16384 + 4, 16384 + 8, 1, 5)
    # no row is carried in: the same calls close nothing in front of the first token
    r = sentences_slice_ref(True, sl, 0, (0, True, False, False, False), SEN_CARRY0)
    assert len(r[0]) == 0 and r[5].tolist() == [0] and r[6][0]
    # a carried row that goes on: its start stays, its end moves
    sl.evl_pos, sl.evl_kind = np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    r = sentences_slice_ref(True, sl, 0, carry, sen)
    assert len(r[0]) == 0 and len(r[5]) == 0 and r[6] == (True, 16000, 16384 + 8, 2, 7 + 6)


def test_the_sentence_calls_check_their_arguments():
    import ctypes as C
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    for name in ("dtk_stream_set_sentences", "dtk_stream_sentences"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert C.sizeof(_lib.StreamSenCarry) == 2 * 4 + 4 * 8
    assert C.sizeof(_lib.StreamSens) == 2 * 8 + 6 * 8 + 2 * 40
    assert L.dtk_stream_set_sentences(None, 1) == _lib.E_ARG
    assert L.dtk_stream_sentences(None, None) == _lib.E_ARG
    h = C.c_void_p()
    if L.dtk_device_count() > 0:
        assert L.dtk_stream_create(16384, 3, C.byref(h)) == _lib.OK
        assert L.dtk_stream_sentences(h, None) == _lib.E_ARG
        assert L.dtk_stream_set_sentences(h, 1) == _lib.OK
        assert L.dtk_stream_set_position_render(h, 1, 12) == _lib.E_ARG      # exclusive, either way round
        ss = _lib.StreamSens()
        assert L.dtk_stream_sentences(h, C.byref(ss)) == _lib.E_STATE        # (outside slice_fn)
        assert L.dtk_stream_set_offsets(h, 1, _lib.SO_BLOCKED) == _lib.OK    # (beside the offsets)
        assert L.dtk_stream_set_offsets(h, 0, 0) == _lib.OK
        assert L.dtk_stream_set_position_render(h, 1, 12) == _lib.E_ARG      # (the rows alone still refuse it)
        assert L.dtk_stream_set_sentences(h, 0) == _lib.OK
        assert L.dtk_stream_set_position_render(h, 1, 12) == _lib.OK
        assert L.dtk_stream_set_sentences(h, 1) == _lib.E_ARG
        assert L.dtk_stream_set_sentences(h, 0) == _lib.OK
        L.dtk_stream_free(h)


def test_python_structs_mirror_the_header(tmp_path):
    """_lib.StreamSenCarry / _lib.StreamSens against the C compiler's layout of dtk_stream_sen_carry / dtk_stream_sens."""
    from datok_amd import _lib
    pairs = (("dtk_stream_sen_carry", _lib.StreamSenCarry), ("dtk_stream_sens", _lib.StreamSens))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "datok_gpu.h"', 'int main(void) {']
    for cname, cls in pairs:
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src.append("return 0; }")
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls)
        for fname, _ in cls._fields_:
            assert int(got[cname + "." + fname]) == getattr(cls, fname).offset, (cname, fname)


_CPP = r'''
#include <cstdio>
#include <fstream>
#include "datok.hpp"
int main(int argc, char **argv) {
  auto loaded = datok::LoadTokenizerFile(argv[1]);
  if (!loaded) return 3;
  auto *tok = static_cast<datok::GpuTokenizer *>(loaded.get());
  std::ifstream in(argv[2], std::ios::binary);
  uint64_t n_tok = 0, n_sen = 0, n_slices = 0;
  const bool ok = tok->TransduceStreamSentences(in, [&](const dtk_stream_slice &sl, const dtk_stream_sens &ss) {
    for (uint64_t i = 0; i < ss.n_sen; i++)
      std::printf("%llu %llu %llu %lld %lld\n", (unsigned long long)(n_tok + ss.sen_tok_end[i]), (unsigned long long)ss.sen_bstart[i],
                  (unsigned long long)ss.sen_bend[i], (long long)ss.sen_rstart[i], (long long)ss.sen_rend[i]);
    n_tok += sl.view.tok_off[1]; n_sen += ss.n_sen; n_slices++;
    return 0;
  }, false, 16384, 3);
  std::printf("%llu rows in %llu slices\n", (unsigned long long)n_sen, (unsigned long long)n_slices);
  return ok ? 0 : 4;
}
'''


def test_cpp_mirror_compiles_and_delivers_the_table(oracle_models, tmp_path):
    """GpuTokenizer::TransduceStreamSentences of include/datok.hpp in a small host program: it compiles and links against
    the header and the library; where a device exists its rows are the stream's table."""
    import datok_amd
    lib = datok_amd.build()
    src, exe = tmp_path / "tss.cpp", tmp_path / "tss"
    src.write_text(_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           lib, "-Wl,-rpath," + os.path.dirname(lib)])
    if datok_amd.lib().dtk_device_count() <= 0:
        return
    om = oracle_models("tokenizer_de.matok")
    raw = sc.running_text(40 * 1024, seed=3)
    inp = tmp_path / "in.txt"
    inp.write_bytes(raw)
    out = subprocess.check_output([str(exe), os.path.join(MODEL_DIR, "tokenizer_de.matok"), str(inp)]).decode().splitlines()
    want = stream_table(sc.oracle_calls(om, raw)[0], om.transduce_doc(raw, 0))
    rows = [tuple(int(x) for x in l.split()) for l in out[:-1]]
    assert rows == list(zip(*(w.tolist() for w in want[:5]))) and len(rows) > 100
    assert out[-1] == "%d rows in 2 slices" % len(rows)      # (the second window reaches the stream's end)
