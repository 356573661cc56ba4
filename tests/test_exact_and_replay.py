"""The exact pass (documents whose calls are not in position order) and the closure replay: call order
and int arguments against the oracle's event list (orc_transduce_events), both encodings.

The crafted tokenizers of tests/craft.py make the reference do what no shipped model does:
consume one EOT twice (double array, datok.go:916-926 + 1019-1030) and fire three epsilon
SentenceEnds at one cursor (matrix.go:573-576)."""
import gzip
import io
import os
import subprocess

import numpy as np
import pytest

import craft
from conftest import MODELS, ROOT
from parity import assert_batch_equals_oracle

from datok_amd.host import _decode_runes

NEWLINE_AFTER_EOT = 16


def _oracle(blob):
    from oracle import oracle as O
    return O.Model(raw=gzip.decompress(blob))


def _write(tmp_path, name, blob):
    path = tmp_path / name
    path.write_bytes(blob)
    return path


def _oracle_calls(om, doc: bytes):
    """[('T', offset, len(buf)) | ('S', arg) | ('E', arg)] in the reference's call order."""
    ev, _ = om.events(doc)
    out = []
    for kind, a, b, c, d in ev:
        if kind == 0:
            out.append(("T", a, len(_decode_runes(doc[b:d])) if d > b else 0, c, d))   # Go's rune count
        else:
            out.append(("SE"[kind - 1], a))
    return out


# ------------------------------------------------------------------ oracle only: the fixtures do what they are for
def test_crafted_models_break_the_position_order_on_the_oracle():
    da = _oracle(craft.datok())
    calls = _oracle_calls(da, b"a\x04a")
    # SentenceEnd(buffc) + TextEnd(0) for the EOT, THEN the token "a" that ends before the EOT, then both again
    assert [c[0] for c in calls] == ["S", "E", "T", "S", "E", "T", "S", "E"]
    assert calls[0] == ("S", 2) and calls[1] == ("E", 0) and calls[2][3:] == (0, 1) and calls[3] == ("S", 1)
    mx = _oracle(craft.matok())
    assert [c[0] for c in _oracle_calls(mx, b"a\x04a")] == ["S", "E", "T", "S", "E"]     # matrix.go:601 rewinds: no revisit
    for blob in (craft.matok(True), craft.datok(True)):
        calls = _oracle_calls(_oracle(blob), b"a. b")
        assert [c[0] for c in calls] == ["T", "T", "S", "S", "S", "T", "S", "E"]


# ------------------------------------------------------------------------------------------------------- GPU
class _Recorder:
    """A custom TokenWriter (token_writer.go:27-33): records every call with its arguments."""

    def __init__(self):
        self.calls = []
        self.Token = lambda off, buf: self.calls.append(("T", off, len(buf)))
        self.SentenceEnd = lambda a: self.calls.append(("S", a))
        self.TextEnd = lambda a: self.calls.append(("E", a))
        self.Flush = lambda: None


def _replayed(res, d, doc: bytes, is_matrix):
    import datok_amd
    from datok_amd import host
    rec = _Recorder()
    if d in res.exact:
        host.replay_calls(doc, res.exact[d], rec)
    else:
        a, b = int(res.tok_off[d]), int(res.tok_off[d + 1])
        host.replay(is_matrix, doc, res.events(d), res.tok_bstart[a:b], rec)
    return rec.calls


@pytest.mark.gpu
@pytest.mark.parametrize("kind,triple", [("datok", False), ("matok", False), ("datok", True), ("matok", True)])
@pytest.mark.parametrize("chunk,flags", [(0, 0), (16, NEWLINE_AFTER_EOT), (None, 0)])
def test_documents_out_of_position_order_are_exact(tmp_path, kind, triple, chunk, flags):
    """Offsets, status, call order, int arguments and rendered bytes of EVERY document equal the oracle's;
    the documents the event bytes cannot express went through the exact pass."""
    import datok_amd
    from datok_amd import corpus
    blob = getattr(craft, kind)(triple)
    path = tmp_path / ("crafted." + kind)
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), _oracle(blob)
    assert tok is not None and tok.type() == kind.upper()
    docs = craft.documents(np.random.default_rng(5))
    text, off = corpus.concat_docs(docs)
    with datok_amd.Batch(max(len(text), 1), len(docs)) as b:
        if chunk is not None:
            b.set_chunking(chunk, 8, extend=0)
        b.set_input(text, off)
        b.run(tok, flags)
        res, tot = b.result(), b.totals()
        assert not any(int(s) & datok_amd.ST_IRREGULAR for s in res.status)
        assert assert_batch_equals_oracle(om, res, text, off, flags) > 100
        if kind == "datok" or triple:
            assert len(res.exact) > 0         # the construct occurred and was handled
        if kind == "matok" and not triple and not flags:
            assert len(res.exact) == 0        # the matrix rewinds at an EOT: nothing to revisit
        # (with NEWLINE_AFTER_EOT the documents with a token that ends at offset 0 go there too: see
        #  test_newline_after_eot_fires_again_at_offset_zero)
        for d, doc in enumerate(docs):
            exp = [c[:3] if c[0] == "T" else c for c in _oracle_calls(om, doc)]
            assert _replayed(res, d, doc, kind == "matok") == exp, (d, doc)
        # the writer's bytes, rendered on the device from the arrays the exact pass wrote
        for bits in (3, 15, 5):
            data, o = b.render(bits | flags)
            for d, doc in enumerate(docs):
                exp, est = om.transduce(doc, bits | flags)
                if est == 0 and not (int(res.status[d]) & ~datok_amd.ST_EMPTY_TEXT):
                    assert data[int(o[d]):int(o[d + 1])] == exp, (bits, d, doc)
    # one stream through the drop-in entry points: device rendering, C++ closure replay, Python closure replay
    for doc in (b"a\x04a", b"a\x04a\x04a\x04a b.", b"a. b.\x04a"):
        for bits in (3, 3 | flags):
            exp, est = om.transduce(doc, bits)
            assert est == 0
            assert tok.transduce_bytes(doc, bits) == (exp, 0)
            assert tok.transduce_bytes(doc, bits, replay=True) == (exp, 0)
        w = io.BytesIO()
        assert tok.transduce_token_writer(io.BytesIO(doc), datok_amd.new_token_writer(w, 3))
        assert w.getvalue() == om.transduce(doc, 3)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_en.matok", "simpletok.datok"])
def test_closure_int_arguments_equal_the_reference(oracle_models, model):
    """SentenceEnd / TextEnd ints: the matrix passes buffc everywhere (matrix.go:575,597,600,684,691), the double
    array 0 (datok.go:1015,1026,1119,1127) except SentenceEnd(buffc) at an EOT (datok.go:1023); Token(offset, buf):
    offset and len(buf).  Python mirror (closure replay) against orc_transduce_events."""
    import datok_amd
    from datok_amd import corpus
    tok, om = datok_amd.load_tokenizer_file(os.path.join(MODELS, model)), oracle_models(model)
    text, off = corpus.german_docs(16, 1024, seed=17)
    raw = text.tobytes()
    docs = [raw[int(off[d]):int(off[d + 1])] for d in range(16)]
    docs += ["This.\n\x04And.\n\x04\n".encode(), "\nThis.\n\x04\nAnd.\n\x04\n".encode(), "Erste.\n\n\n\n\x04\nNächst.\x04".encode(),
             "word\x04 more words. And\x04more".encode(), b"a\x04b\x04c", "„Zitat“ – so … »y« 日本語".encode(), b"", b" ", b"\x04",
             b"Hallo! " + b"w" * 64 + b" Ende.", b"x" * 40 + b". Und   \n\n weiter ...", b"\xff\xfe bad \x80 bytes \xc3"]
    n_args = 0
    for doc in docs:
        rec = _Recorder()
        assert tok.transduce_token_writer(io.BytesIO(doc), rec)
        exp = [c[:3] if c[0] == "T" else c for c in _oracle_calls(om, doc)]
        assert rec.calls == exp, (model, doc[:60])
        n_args += sum(1 for c in exp if c[0] != "T" and c[1] != 0)
    if model.endswith(".matok"):
        assert n_args > 10       # nonzero where the window holds runes: EOT texts, leading blanks, the tail


@pytest.mark.gpu
def test_closure_int_arguments_cpp_mirror(oracle_models, tmp_path):
    """The same through include/datok.hpp (TransduceTokenWriter with a custom writer)."""
    import datok_amd
    lib = datok_amd.build()
    src = tmp_path / "args.cpp"
    src.write_text(r'''
#include <fstream>
#include <iostream>
#include "datok.hpp"
int main(int argc, char **argv) {
  auto tok = datok::LoadTokenizerFile(argv[1]);
  if (!tok) return 3;
  std::ifstream in(argv[2], std::ios::binary);
  datok::TokenWriter tw;
  tw.Token = [&](int off, const std::vector<datok::rune> &buf) { std::cout << "T " << off << " " << buf.size() << "\n"; };
  tw.SentenceEnd = [&](int a) { std::cout << "S " << a << "\n"; };
  tw.TextEnd = [&](int a) { std::cout << "E " << a << "\n"; };
  tw.Flush = [] { return 0; };
  return tok->TransduceTokenWriter(in, tw) ? 0 : 5;
}
''')
    exe = tmp_path / "args"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           lib, "-Wl,-rpath," + os.path.dirname(lib)])
    doc = "Der alte Mann. Er ging!\n\x04\nNoch ein Text, z.B. hier.\x04 Ende".encode()
    inp = tmp_path / "in.txt"
    inp.write_bytes(doc)
    models = [(os.path.join(MODELS, m), oracle_models(m)) for m in ("tokenizer_de.matok", "tokenizer_de.datok")]
    for kind in ("datok", "matok"):                 # and a crafted one whose calls come from the exact pass
        p = tmp_path / ("crafted." + kind)
        p.write_bytes(getattr(craft, kind)())
        models.append((str(p), _oracle(getattr(craft, kind)())))
    for i, (path, om) in enumerate(models):
        if i >= 2:
            inp.write_bytes(b"ab a\x04a\x04a. b\x04ab")
            doc = inp.read_bytes()
        r = subprocess.run([str(exe), path, str(inp)], capture_output=True)
        assert r.returncode == 0, r.stderr
        got = [tuple([ln.split()[0]] + [int(x) for x in ln.split()[1:]]) for ln in r.stdout.decode().splitlines()]
        exp = [c[:3] if c[0] == "T" else c for c in _oracle_calls(om, doc)]
        assert got == exp, path


@pytest.mark.gpu
def test_crafted_models_through_the_two_launch_first_pass():
    """DATOK_SPLIT_START=1 (start records and chunk walk as two launches, windows chained from the first pass on:
    what a batch with chunks of more than 256 bytes runs, and what every repair round runs).  A double-array lane
    may fire an EOT behind its stop position and then backtrack to a token end in front of it; dropped as out of
    its window, that event made the lane fail its check in every repair round (EventSink::eot) -- the rounds spun
    for 90 s.  Every test of this file through that path."""
    import sys
    e = dict(os.environ); e["DATOK_SPLIT_START"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                        "not two_launch", os.path.abspath(__file__)], capture_output=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and b" passed" in r.stdout, (r.stdout.decode()[-1500:], r.stderr.decode()[-500:])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["matok", "datok"])
def test_newline_after_eot_fires_again_at_offset_zero(tmp_path, kind):
    """token_writer.go:66-68 decrements posC whenever it is 0 and the buffer starts with a newline -- not only for a
    text's first token.  A tokenizer that makes a token of the newline itself (the crafted ones do) yields a first
    token [-1, 0) behind an EOT, posC is 0 again, and the rule fires a second time if the next buffer starts with a
    newline too.  The compaction models the rule as one shift per text and leaves a document with a token that ends at
    offset 0 to the exact pass (scripts/crafted_sweep.py found it: offsets one too high behind such a token)."""
    import datok_amd
    from datok_amd import corpus
    blob = getattr(craft, kind)(False)
    path = tmp_path / ("crafted." + kind)
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), _oracle(blob)
    docs = [b"aba \x04\na aaabb\n \x04b a\n\na  b\n  \nb\x04\n\nab .   a aa", b"b\x04\n\nab", b"a\x04\n\n\na b\x04\n\nb",
            b"\n\na", b"ab\x04\nab\x04\n\n\nab"] * 3
    text, off = corpus.concat_docs(docs)
    for chunk, warm in ((0, 0), (16, 0), (16, 8), (24, 2), (None, 16)):
        with datok_amd.Batch(len(text), len(docs)) as b:
            if chunk is not None:
                b.set_chunking(chunk, warm, extend=0)
            b.set_input(text, off)
            for _ in range(2):
                b.run(tok, NEWLINE_AFTER_EOT)
                assert assert_batch_equals_oracle(om, b.result(), text, off, NEWLINE_AFTER_EOT) >= 5
            # the offset -1 of that first token in the narrow form of the rune offsets (DTK_R_TOK_RUNE16)
            b.set_result_fields(datok_amd.Batch.R_ALL | datok_amd.Batch.R_TOK_RUNE16)
            r = b.result()
            assert int(r.tok_rstart.min()) == (-1 if kind == "matok" else 0) and r.tok_r16.dtype == np.int16
            assert np.array_equal(r.tok_r16[:, 0], r.tok_rstart) and np.array_equal(r.tok_r16[:, 1], r.tok_rend)


# the automata scripts/fuzz_automata.py found a fault with (seed -> what it was), plus a few that never failed
FUZZ_SEEDS = {
    1: "a hard fail on the document's last rune, an EOT, leaves `eot` set: the lane that read it runs the EOF drain",
    5: "a fused cell taken behind the token start (bufft > buffc after a backtrack) neither flushes nor rewinds",
    6: "double array: a token flushed after an EOT's TextEnd that ends before it",
    9: "the stale `eot` fires behind a Token that ends at the same position: rows in call order",
    14: "matrix.go:593-605 fires after ANY successful step while `eot` is set -- also an epsilon step of the EOF drain",
    63: "SentenceEnd calls at positions 1, 0, 1 (EOF drain, popped epsilon slot): twice at one position, not adjacent",
    2: None, 3: None, 100: None, 1000: None,
}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sorted(FUZZ_SEEDS))
def test_random_automata_equal_the_oracle(tmp_path, seed):
    """Random arc tables in both file formats x random documents x chunkings x flags: offsets, status and the writer's
    rendered output of every document against the oracle.  The shipped models only do what real tokenizers do; these
    reach the reference's odd corners (see FUZZ_SEEDS; scripts/fuzz_automata.py runs thousands)."""
    import datok_amd
    from datok_amd import corpus
    rng = np.random.default_rng(seed)
    arcs = craft.random_automaton(rng)
    docs = craft.random_documents(rng) + [b" \x04", b"a \x04", b"bx \nb\x04", b"\n", b"\n\n",
                                          b"ab\n\nba\nbb.\x04\x04 \n\n.\nab .\n\x04\x04..ba \nbb\x04"]
    text, off = corpus.concat_docs(docs)
    compared = 0
    for kind in ("matok", "datok"):
        blob = getattr(craft, kind + "_from")(arcs)
        path = tmp_path / ("fuzz." + kind)
        path.write_bytes(blob)
        tok, om = datok_amd.load_tokenizer_file(str(path)), _oracle(blob)
        assert tok is not None
        for chunk, warm in ((0, 0), (16, 0), (16, 8), (32, 4), (None, 16)):
            for flags in (0, NEWLINE_AFTER_EOT):
                with datok_amd.Batch(len(text), len(docs)) as b:
                    if chunk is not None:
                        b.set_chunking(chunk, warm, extend=0 if warm < 8 else 16)
                    b.set_input(text, off)
                    b.run(tok, flags)
                    res = b.result()
                    compared += assert_batch_equals_oracle(om, res, text, off, flags)
                    if chunk in (0, 16) and warm == 0:
                        for bits in (3, 15):
                            data, o = b.render(bits | flags)
                            for d, doc in enumerate(docs):
                                exp, est = om.transduce(doc, bits | flags)
                                if est == 0 and not (int(res.status[d]) & ~datok_amd.ST_EMPTY_TEXT):
                                    assert bytes(data[int(o[d]):int(o[d + 1])]) == exp, (kind, chunk, flags, bits, doc)
    assert compared > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["matok", "datok"])
def test_symbol_stream_of_entries_for_a_sigma_beyond_the_code_table(tmp_path, kind):
    """The symbol stream holds one code per input byte where the model's distinct entries fit a byte (the shipped
    tokenizers: some 170 symbols, 200 entries; `dtk_model_info.stream_codes`), else the 16-bit entries themselves,
    walked by the general loop.  A tokenizer with 300 more characters in its sigma takes that path; arcs on some of
    them, documents that mix them with the usual letters, invalid bytes and runes outside the sigma."""
    import datok_amd
    from datok_amd import corpus
    rng = np.random.default_rng(7)
    blob, extra = craft.big_sigma(kind)  # forty of the new characters are letters like "a"
    path = tmp_path / ("big." + kind)
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), _oracle(blob)
    assert tok is not None and tok.info["stream_codes"] == 0, tok.info
    small = datok_amd.load_tokenizer_file(os.path.join(MODELS, "tokenizer_de.matok"))
    if not os.environ.get("DATOK_SYM16"):      # (the switch that forces 16-bit entries for every model)
        assert 0 < small.info["stream_codes"] < 255, small.info
    raw = [c.encode() for c in extra[:40]] + [b"\xff", b"\xe4\xb8", "鿿".encode(), "\U0001F600".encode()]
    docs = craft.random_documents(rng, 200, 120, raw)
    text, off = corpus.concat_docs(docs)
    compared = 0
    for chunk, warm in ((0, 0), (16, 4), (None, 16)):
        with datok_amd.Batch(len(text), len(docs)) as b:
            if chunk is not None:
                b.set_chunking(chunk, warm, extend=0)
            b.set_input(text, off)
            b.run(tok, 0)
            res = b.result()
            compared += assert_batch_equals_oracle(om, res, text, off, 0)
            data, o = b.render(3)
            for d, doc in enumerate(docs):
                exp, est = om.transduce(doc, 3)
                if est == 0 and not (int(res.status[d]) & ~datok_amd.ST_EMPTY_TEXT):
                    assert bytes(data[int(o[d]):int(o[d + 1])]) == exp, (chunk, doc)
    assert compared > 50


@pytest.mark.gpu
def test_converted_double_array_on_the_device(tmp_path):
    """`datok convert --double-array` (dtk_foma_to_datok, host code) of the shipped tokenizer_de.fst, loaded like any
    .datok file (dense layout and all) and walked on the device: every offset equal to the oracle's walk of the same
    image, and -- no U+0004 in these documents -- to the matrix tokenizer's result."""
    import datok_amd
    from datok_amd import corpus
    with open(os.path.join(MODELS, "tokenizer_de.fst"), "rb") as f:
        img = datok_amd.foma_to_datok(f.read())
    path = tmp_path / "converted.datok"
    path.write_bytes(img)
    tok, om = datok_amd.load_tokenizer_file(str(path)), _oracle(img)
    assert tok.type() == "DATOK"
    if not any(os.environ.get(k) for k in ("DATOK_NO_DENSE", "DATOK_NO_FUSED", "DATOK_FORCE_WIDE")):
        assert tok.info["dense_states"] > 0
    text, off = corpus.german_docs(256, 2048, seed=21)
    mat = datok_amd.load_tokenizer_file(os.path.join(MODELS, "tokenizer_de.matok"))
    with datok_amd.Batch(len(text), len(off) - 1) as b, datok_amd.Batch(len(text), len(off) - 1) as bm:
        b.set_input(text, off); bm.set_input(text, off)
        b.run(tok, 0); bm.run(mat, 0)
        res, resm = b.result(), bm.result()
        assert assert_batch_equals_oracle(om, res, text, off, 0) == len(off) - 1
        for k in ("tok_off", "sent_off", "tok_rstart", "tok_rend", "tok_bstart", "tok_bend", "sent"):
            assert np.array_equal(getattr(res, k), getattr(resm, k)), k


@pytest.mark.gpu
def test_double_array_with_slots_behind_its_size(tmp_path):
    """ADVICE r02.  datok.go:876 probes a state's epsilon slot without the size bound that datok.go:896 puts on every
    transition: in a hand-made (or truncated) file a state can "have" an epsilon arc -- a remembered slot to backtrack
    to -- that no transition can take.  ToDoubleArray never writes such a file and the reference holds none (parity
    unpinned, the oracle is the restatement); the dense layout does not apply to one (the pairs are walked) and the
    result must equal the oracle's either way."""
    import datok_amd
    from datok_amd import corpus
    rng = np.random.default_rng(77)
    docs = craft.documents(rng, 200) + craft.random_documents(rng, 100)
    text, off = corpus.concat_docs(docs)
    fell_back = compared = 0
    for arcs in (craft._automaton(False), craft.random_automaton(np.random.default_rng(14))):
        whole = datok_amd.load_tokenizer_file(str(_write(tmp_path, "whole.datok", craft.datok_from(arcs))))
        for cut in (1, 4, 9, 14, 20):
            blob = craft.datok_from(arcs, size_cut=cut)
            tok, om = datok_amd.load_tokenizer_file(str(_write(tmp_path, "cut%d.datok" % cut, blob))), _oracle(blob)
            assert tok is not None
            if whole.info["dense_states"] and not tok.info["dense_states"]:
                fell_back += 1
            for chunk in (0, 16):
                with datok_amd.Batch(len(text), len(docs)) as b:
                    b.set_chunking(chunk, 8, extend=0)
                    b.set_input(text, off)
                    b.run(tok, 0)
                    # (ST_BAD_MODEL: at the end of a document such a state makes the reference take an epsilon step that
                    #  fails with nothing buffered -- it then emits a rune from behind its buffer's fill mark,
                    #  datok.go:942-951; the library flags the document instead of inventing that rune)
                    compared += assert_batch_equals_oracle(om, b.result(), text, off, 0, skip_status=datok_amd.ST_BAD_MODEL)
    assert compared > 1000
    if not any(os.environ.get(k) for k in ("DATOK_NO_DENSE", "DATOK_NO_FUSED", "DATOK_FORCE_WIDE")):
        assert fell_back > 0   # (some cut put an epsilon slot behind the size: no dense layout for that file)
