"""One stream of any length in slices cut at verified sync points (dtk_stream_run) on the GPU:
every call of every stream is compared with the oracle's calls for the WHOLE stream -- Token window start, start and
end in stream bytes, and the ints of SentenceEnd / TextEnd -- and the mirrors' bytes with the oracle's."""
import io
import os
import subprocess
import sys

import pytest

import bigsigma
import craft
import streamcorpus as sc
from conftest import MODELS, ROOT

pytestmark = pytest.mark.gpu

S, T = sc.S, sc.T
_FATAL = 1 | 4 | 16 | 32 | 8


@pytest.fixture(scope="module")
def models():
    """name -> (device tokenizer, oracle model), as bigsigma.device_model names them: "tokenizer_de.datok:pairs" is the
    double array walked as pairs, "<file>:entries" a stream of 16-bit entries on the lean loop, "<file>:entries-general"
    the same stream on the general loop, "de64.matok" the enlarged model, which has such a stream by itself."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bigsigma.device_model(name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def whole():
    """lang -> (the 200 KB stream of test 1, per oracle model name its calls and status), computed once."""
    texts, calls = {}, {}

    def get(lang, name, om):
        if lang not in texts:
            texts[lang] = sc.running_text(200 * 1024, seed=5, lang=lang)
        if name not in calls:
            calls[name] = sc.oracle_calls(om, texts[lang])
        return texts[lang], calls[name][0], calls[name][1]
    return get


def run_stream(st, tok, raw, read_size=None):
    """(slices, status) of one run; read_size: the reader hands out at most that many bytes a call."""
    r = io.BytesIO(raw)
    if read_size:
        class Short:
            def read(self, n):
                return r.read(min(n, read_size))
        reader = Short()
    else:
        reader = r
    slices = []
    status = st.run(tok, reader, on_slice=slices.append)
    return slices, status


def assert_stream(st, tok, om, raw, expect=None, read_size=None, slice_bytes=S):
    calls, ost = expect if expect is not None else sc.oracle_calls(om, raw)
    slices, status = run_stream(st, tok, raw, read_size)
    sc.check_slices(slices, len(raw), slice_bytes)
    got = sc.stream_calls(om.type() == "MATOK", slices)
    if ost & sc.ST_WINDOW_OVERFLOW:
        # The reference panics where its window overflows (matrix.go:365,406), and the walk ends the stream there with
        # a TextEnd (DTK_WINDOW_BYTES): the calls in front of the token that does not fit a window are the stream's.
        n = next(i for i, c in enumerate(calls) if c[0] == 0 and c[4] - c[2] > 4104)
        assert n > 100 and len(got) >= n
        got, calls = got[:n], calls[:n]
    if got != calls:
        i = next((i for i, (a, b) in enumerate(zip(got, calls)) if a != b), min(len(got), len(calls)))
        raise AssertionError("call %d of %d / %d: got %r, oracle %r" % (i, len(got), len(calls), got[i:i + 3], calls[i:i + 3]))
    assert status == ost, (status, ost)
    assert status == 0 or any(s.status for s in slices)
    return slices


MODELS_1 = ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_de.datok:pairs", "tokenizer_en.matok"]
# the same automata over a stream of 16-bit entries: the lean loop, the double array's dense layout, the general loop
MODELS_ENTRIES = ["tokenizer_de.matok:entries", "tokenizer_de.datok:entries", "tokenizer_de.matok:entries-general"]


# ---- 1. the stream itself
@pytest.mark.parametrize("name", MODELS_1 + MODELS_ENTRIES)
def test_stream_calls_equal_the_oracles(models, whole, name):
    import datok_amd
    tok, om = models(name)
    raw, calls, ost = whole("en" if "_en" in name else "de", name.partition(":")[0], om)
    assert ost == 0 and raw.count(b"\x04") >= 10
    with datok_amd.Stream(S) as st:
        slices = assert_stream(st, tok, om, raw, (calls, ost))
        assert len(slices) >= 12
        if name in MODELS_ENTRIES:           # (how the reader hands out bytes and the depth do not meet the stream's format)
            return
        assert_stream(st, tok, om, raw, (calls, ost), read_size=5000)        # short reads are retried
    with datok_amd.Stream(S, depth=2) as st:
        assert_stream(st, tok, om, raw, (calls, ost))


def test_stream_calls_of_the_enlarged_model(models, whole):
    """A model with more than 255 entries (bigsigma.enlarged_de): slices cut at verified sync points and the state
    carried from slice to slice over 16-bit entries, on German text with the new characters spliced in -- letters, sentence
    ends and blanks among them -- and on the same kind of text with bytes that do not decode."""
    import datok_amd
    import numpy as np
    from test_stream_render import invalid_stream_spliced
    tok, om = models("de64.matok")
    german = whole("de", "tokenizer_de.matok", models("tokenizer_de.matok")[1])[0]
    spliced = bigsigma.splice(german.replace(b"\x04", b" "), np.random.default_rng(3), limit=4 * S)
    assert sum(spliced.count(c.encode()) for c in bigsigma.CHARS) >= 1000
    with datok_amd.Stream(S) as st:
        for raw in (spliced, invalid_stream_spliced()):
            calls, ost = sc.oracle_calls(om, raw)
            assert ost == 0
            slices = assert_stream(st, tok, om, raw, (calls, ost))
            assert len(slices) >= 4


@pytest.mark.parametrize("name", MODELS_1)
def test_mirrors_write_the_oracles_bytes_in_every_mode(models, whole, name):
    """The C++ mirror (dtk_stream_transduce) and the Python mirror, slice by slice into one writer."""
    import datok_amd
    from datok_amd import host
    tok, om = models(name)
    raw = whole("en" if "_en" in name else "de", name.partition(":")[0], om)[0]
    is_matrix = tok.type() == "MATOK"
    with datok_amd.Stream(S) as st:
        slices, _ = run_stream(st, tok, raw)
        for nl in (0, host.NEWLINE_AFTER_EOT):
            for mode in sc.MODES:
                exp, est = om.transduce(raw, mode | nl)
                assert st.transduce(tok, raw, mode | nl) == (exp, est), (mode, nl)
                w = io.BytesIO()
                tw = host.new_token_writer(w, mode | nl)
                for sl in slices:
                    host.replay_slice(is_matrix, sl, tw)
                tw.Flush()
                assert w.getvalue() == exp, (mode, nl)
    w = io.BytesIO()
    assert tok.transduce_token_writer(io.BytesIO(raw), host.new_token_writer(w, host.SIMPLE), slice_bytes=S)
    assert w.getvalue() == om.transduce(raw, host.SIMPLE)[0] and tok.last_status == 0


# ---- 2. every alignment of a cut
CUT_CASES = ([(c, n) for c in sc.CONSTRUCTS for n in ("tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_de.datok:pairs")]
             + [(c, "tokenizer_de.matok:entries") for c in ("token300", "token4000")])


@pytest.mark.parametrize("construct,name", CUT_CASES)
def test_every_alignment_of_a_cut(models, name, construct):
    """(Over 16-bit entries: the two long tokens, whose carried position lies far into the tail, at three shifts.)"""
    import datok_amd
    from datok_amd import host
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for shift in (range(41) if ":entries" not in name else (0, 1, 39)):
            raw = sc.construct_stream(construct, shift)
            slices = assert_stream(st, tok, om, raw)
            if construct == "token5000":
                assert slices[-1].status & sc.ST_WINDOW_OVERFLOW
            elif construct == "token4000" and shift < 8:
                assert slices[1].first > 3900                     # the carried position near the tail's end
            if construct.startswith("eot") and shift in (0, 1, 2, 39):
                flags = host.TOKENS | host.SENTENCES | host.TOKEN_POS | host.SENTENCE_POS | host.NEWLINE_AFTER_EOT
                assert st.transduce(tok, raw, flags) == om.transduce(raw, flags), shift


# ---- 3. chunk and warm-up settings
@pytest.mark.parametrize("chunk", [16, 64, 256, 0])
@pytest.mark.parametrize("warm", [0, 8])
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_chunk_and_warm_up_settings(models, whole, name, chunk, warm):
    """Warm-up 0 forces repair rounds; chunk 0 is the walk with one lane per slice."""
    import datok_amd
    tok, om = models(name)
    raw, calls, ost = whole("de", name, om)
    with datok_amd.Stream(S) as st:
        st.set_chunking(chunk, warm)
        assert_stream(st, tok, om, raw, (calls, ost))


@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_round_limit_falls_back_to_one_lane_per_slice(models, whole, name):
    import datok_amd
    tok, om = models(name)
    raw, calls, ost = whole("de", name, om)
    assert datok_amd.lib().dtk_debug_configure(b"ROUND_LIMIT", b"1") == 0
    try:
        st = datok_amd.Stream(S)
    finally:
        assert datok_amd.lib().dtk_debug_configure(b"ROUND_LIMIT", os.environ.get("DATOK_ROUND_LIMIT", "-1").encode()) == 0
    with st:
        st.set_chunking(16, 0)         # (no warm-up: more repair rounds than the limit allows)
        assert_stream(st, tok, om, raw, (calls, ost))


# ---- 4. boundary stream lengths
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_boundary_stream_lengths(models, name):
    import datok_amd
    tok, om = models(name)
    text = sc.running_text(2 * S + T + 64, seed=8)
    with datok_amd.Stream(S) as st:
        for n in (0, 1, S, S + T, S + T + 1, 2 * S):
            b = bytearray(text[:n])
            i = n - 1
            while i >= 0 and b[i] >= 0x80:       # (no rune cut in two at the end)
                b[i] = ord("x")
                i -= 1
            raw = bytes(b)
            assert len(raw) == n
            slices = assert_stream(st, tok, om, raw)
            assert len(slices) == (1 if n <= S + T else 2), n


# ---- a text that spans a cut: DTK_ST_EMPTY_TEXT is the stream's to decide
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_empty_text_is_decided_across_cuts(models, name):
    import datok_amd
    tok, om = models(name)
    fill = sc.running_text(3 * S, seed=4).replace(b"\x04", b" ")
    with datok_amd.Stream(S) as st:
        for chunk in (0xFFFFFFFF, 0):
            st.set_chunking(chunk, 8)
            for shift in range(0, 24, 3):
                left = fill[:S - 12 + shift]
                left = left[:left.rfind(b" ")] + b". "
                # the text's last token lies in front of the cut, its SentenceEnd / TextEnd behind it: not empty
                raw = left + b" " * 40 + b"\x04\nWeiter geht es. " + fill[:S]
                assert sc.oracle_calls(om, raw)[1] == 0
                assert_stream(st, tok, om, raw)
                # an empty text behind the cut, and one around it
                for extra in (b" " * 40 + b"\x04 \x04\nWeiter. ", b"\x04" + b" " * 40 + b"\x04\nWeiter. "):
                    raw = left + extra + fill[:S]
                    assert sc.oracle_calls(om, raw)[1] == sc.ST_EMPTY_TEXT
                    assert_stream(st, tok, om, raw)


# ---- 5. reuse
def test_one_stream_object_twice(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    a, b = sc.running_text(50000, seed=1), sc.running_text(70000, seed=2)
    with datok_amd.Stream(S) as st:
        assert_stream(st, tok, om, a)
        assert_stream(st, tok, om, b)
        assert_stream(st, tok, om, a)


# ---- 6. a crafted model whose slice needs the exact pass
def test_crafted_double_array_is_refused(tmp_path):
    import datok_amd
    from datok_amd import _lib, host
    from oracle import oracle as O
    img = craft.datok()
    path = tmp_path / "revisit.datok"
    path.write_bytes(img)
    tok = datok_amd.load_tokenizer_file(str(path))
    import gzip
    om = O.Model(raw=gzip.decompress(img))
    raw = (b"ab ab. " * 40 + b"a\x04a ") * 120                 # the double array consumes every such EOT twice
    assert len(raw) > 2 * S
    with datok_amd.Stream(S) as st:
        with pytest.raises(_lib.DatokGpuError) as e:
            st.run(tok, raw)
        assert e.value.code == _lib.E_IRREGULAR
        assert st.run(tok, b"ab ab. " * 3000) == 0              # the object is still good
    for flags in (host.SIMPLE, 15):
        assert tok.transduce_bytes(raw, flags, replay=True)[0] == om.transduce(raw, flags)[0]


# ---- 7. the command line
def test_cli_reads_a_file_and_stdin_as_one_stream(models, tmp_path):
    tok, om = models("tokenizer_de.matok")
    raw = sc.running_text(300 * 1024, seed=12)
    exp, st = om.transduce(raw, 3)
    assert st == 0
    f = tmp_path / "in.txt"
    f.write_bytes(raw)
    cli = os.path.join(ROOT, "datok_amd", "datok")
    cmd = [cli, "tokenize", "-t", os.path.join(MODELS, "tokenizer_de.matok"), "--slice-bytes", "16384"]
    out = subprocess.run(cmd + [str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == exp
    out = subprocess.run(cmd + ["-"], input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == exp
    bad = subprocess.run(cmd[:-1] + ["1000", str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert bad.returncode != 0 and b"invalid argument" in bad.stderr.lower()
    assert sys.getsizeof(exp) > 0
