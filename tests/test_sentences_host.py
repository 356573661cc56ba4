"""The sentence table (DTK_R_SENTENCES, dtk_sentence_view of include/datok_gpu.h), CPU tier: the definition of
tests/sentences.py on hand-worked call lists and against the oracle's calls and writer, the ctypes mirror of the view,
and datok::sentence_rows of include/datok.hpp in a stand-alone host program.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import blocked
import sentences
from conftest import ROOT
from test_event_list import _edge_documents
from test_host_logic import TEXTS, matrix_events

T, S, E = ("T",), ("S",), ("E",)


def test_from_calls_on_hand_worked_call_lists():
    fc = sentences.from_calls
    assert fc([T, T, S, S, T, S]) == ([0, 2], 3)                  # two SentenceEnds in a row: no row between them
    assert fc([T, T, E, T, S, E]) == ([0, 2], 3)                  # a TextEnd closes the open sentence
    assert fc([T, S, T, T]) == ([0, 1], 3)                        # tokens with no closing call
    assert fc([S, E]) == ([], 0) and fc([]) == ([], 0)            # a document with no token
    assert fc([T, S, E, S, E, T]) == ([0, 1], 2)                  # an EOT text with no token, between two others
    assert fc([S, T, T]) == ([0], 2)                              # a boundary in front of the first token
    # the oracle's rows (kind, a, b, c, d) and the C-ABI's (kind, a, b, c) count the same
    assert fc([(0, 0, 0, 0, 2), (1, 0, 0, 0, 0), (0, 1, 2, 3, 5), (2, 0, 0, 0, 0)]) == ([0, 1], 2)


def test_rows_of_gathers_first_and_last_token():
    r = sentences.rows_of([0, 2], 3, [0, 3, 6], [2, 5, 9], [0, 3, 0], [2, 5, 3], text_tok_end=[2, 3])
    assert r["sen_tok_end"].tolist() == [2, 3] and r["sen_tok_end"].dtype == np.uint32
    assert r["sen_bstart"].tolist() == [0, 6] and r["sen_bend"].tolist() == [5, 9]
    assert r["sen_rstart"].tolist() == [0, 0] and r["sen_rend"].tolist() == [5, 3] and r["sen_rend"].dtype == np.int32
    assert r["text_sen_end"].tolist() == [1, 2]                   # rows whose first token is < text_tok_end
    r = sentences.rows_of([], 0, [], [], text_tok_end=[0])
    assert r["sen_tok_end"].tolist() == [] and r["text_sen_end"].tolist() == [0] and r["sen_rstart"] is None


def _documents():
    eot = [d for d in _edge_documents() if b"\x04" in d]
    assert len(eot) > 100
    return [t.encode() for t in TEXTS] + blocked.five_documents() + eot


@pytest.mark.parametrize("model", ["tokenizer_de.matok", "tokenizer_en.matok", "tokenizer_de.datok"])
def test_definition_against_the_oracle(oracle_models, model):
    """from_calls on the oracle's calls: as many rows as the writer's Token closure pushes ints to sent[] (every
    SentenceEnd call pushes one more, token_writer.go:108), so at most len(sent); and, for the matrix models, the rows
    of the one-bit machine run over matrix_events' bytes."""
    om = oracle_models(model)
    total = checked = 0
    for raw in _documents():
        calls, _ = om.events(raw)
        firsts, n_tok = sentences.from_calls(calls)
        exp = om.transduce_doc(raw, 0)
        assert n_tok == len(exp.tok_bend), raw[:40]
        total += len(firsts)
        if exp.status == 0:
            pushes = len(exp.sent) - sum(1 for c in calls if c[0] == 1)
            assert len(firsts) == pushes <= len(exp.sent), raw[:40]
            checked += 1
        if model.endswith(".matok") and not exp.status & 1:
            ev, _ = matrix_events(om, raw)
            cursors = sentences.machine(ev)
            assert [int(exp.tok_bend[f]) for f in firsts] == cursors, raw[:40]
    print("%s: %d sentences, %d documents with the writer's count" % (model, total, checked))
    assert total > 3000 and checked > 100


def test_python_struct_mirrors_the_header(tmp_path):
    """_lib.SentenceView against the C compiler's layout of dtk_sentence_view."""
    from datok_amd import _lib
    cname, cls = "dtk_sentence_view", _lib.SentenceView
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "datok_gpu.h"', 'int main(void) {',
           'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in cls._fields_:
        src.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    src.append('printf("bit %d\\n", (int)DTK_R_SENTENCES);')
    src.append("return 0; }")
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) and len(cls._fields_) == 8
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname
    import datok_amd
    assert int(got["bit"]) == datok_amd.Batch.R_SENTENCES and not datok_amd.Batch.R_SENTENCES & (datok_amd.Batch.R_ALL | 4096)
    assert {"dtk_batch_sentences_device", "dtk_batch_sentences_host"} <= set(_lib.EXPORTS)


_CPP = r'''
#include <cstdio>
#include "datok.hpp"
int main() {
  // three documents: two rows, none, one row; the second view has no rune offsets
  const uint64_t off[] = {0, 2, 2, 3};
  const uint32_t tok_end[] = {2, 5, 1}, bs[] = {0, 9, 3}, be[] = {8, 30, 4}, tse[] = {1};
  const int32_t rs[] = {0, -1, 3}, re[] = {8, 28, 4};
  dtk_sentence_view v{3, off, tok_end, bs, be, rs, re, tse};
  for (int pass = 0; pass < 2; pass++) {
    for (uint32_t d = 0; d < 3; d++) {
      const std::vector<datok::SentenceRow> rows = datok::sentence_rows(v, d);
      std::printf("%u:", d);
      for (const datok::SentenceRow &r : rows)
        std::printf(" [%u,%u) b[%u,%u) r[%d,%d)", r.tok_first, r.tok_end, r.bstart, r.bend, r.rstart, r.rend);
      std::printf("\n");
    }
    v.sen_rstart = v.sen_rend = nullptr;
  }
  return 0;
}
'''


def test_cpp_sentence_rows(tmp_path):
    """datok::sentence_rows of include/datok.hpp in a stand-alone host program on a hand-built view."""
    src, exe = tmp_path / "sr.cpp", tmp_path / "sr"
    src.write_text(_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().splitlines()
    assert out[:3] == ["0: [0,2) b[0,8) r[0,8) [2,5) b[9,30) r[-1,28)", "1:", "2: [0,1) b[3,4) r[3,4)"]
    assert out[3:] == ["0: [0,2) b[0,8) r[0,0) [2,5) b[9,30) r[0,0)", "1:", "2: [0,1) b[3,4) r[0,0)"]
