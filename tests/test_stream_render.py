"""A stream's token and sentence text rendered on the device (dtk_stream_set_render, dtk_streamrender.hip): in the four
position-free writer modes every slice brings the bytes a stock NewTokenWriter writes for its calls.  Every test compares
the slices' bytes, one after the other, with the oracle's bytes for the WHOLE stream, and every slice's bytes with
streamrender.render_slice_ref of that slice's own arrays, so that a failure names the slice."""
import io
import os
import subprocess

import numpy as np
import pytest

import bigsigma
import streamcorpus as sc
from conftest import MODELS, ROOT
from streamrender import FFFD, render_slice_ref
from test_stream import models, whole  # noqa: F401  (fixtures: the device and oracle models, the 200 KB streams)

pytestmark = pytest.mark.gpu

S = sc.S
MODES = (0, 1, 2, 3)
NL = 16


def run_rendered(st, tok, raw, read_size=None):
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


def calls_bytes(calls, mode):
    """Bytes a position-free writer writes for a list of the oracle's calls over valid UTF-8."""
    return sum((c[4] - c[3] + 1 if mode & 1 else 0) if c[0] == 0 else (1 if c[0] == 2 or mode & 2 else 0) for c in calls)


def assert_rendered(st, tok, om, raw, mode, read_size=None, exp=None):
    """Renders `raw` in `mode` on `st`; returns the slices."""
    is_matrix = tok.type() == "MATOK"
    st.set_render(mode)
    slices, status = run_rendered(st, tok, raw, read_size)
    sc.check_slices(slices, len(raw))
    for i, sl in enumerate(slices):
        assert sl.out is not None, i
        ref = render_slice_ref(is_matrix, sl, mode)
        if sl.out != ref:
            k = next((j for j, (a, b) in enumerate(zip(sl.out, ref)) if a != b), min(len(sl.out), len(ref)))
            raise AssertionError("slice %d of %d (base %d, %d tokens, %d entries): %d bytes against %d, first difference at %d: "
                                 "%r against %r" % (i, len(slices), sl.base, len(sl.tok_bend), len(sl.evl_pos), len(sl.out),
                                                    len(ref), k, sl.out[max(k - 20, 0):k + 20], ref[max(k - 20, 0):k + 20]))
    got = b"".join(sl.out for sl in slices)
    if exp is None:
        exp = om.transduce(raw, mode)[0]
    if status & sc.ST_WINDOW_OVERFLOW:
        # The reference panics where its window overflows, and the walk ends the stream there: the calls in front of the
        # token that fits no window are the stream's (test_stream.py, assert_stream), and so are their bytes.
        calls = sc.oracle_calls(om, raw)[0]
        n = next(i for i, c in enumerate(calls) if c[0] == 0 and c[4] - c[2] > 4104)
        k = calls_bytes(calls[:n], mode)
        assert n > 100 and len(got) >= k
        got, exp = got[:k], exp[:k]
    assert len(got) == len(exp), (mode, len(got), len(exp))
    assert got == exp, mode
    return slices


MODELS_1 = ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_de.datok:pairs", "tokenizer_en.matok"]


# ---- 1. the 200 KB streams
@pytest.mark.parametrize("name", MODELS_1)
def test_rendered_stream_equals_the_oracles_bytes(models, whole, name):
    import datok_amd
    tok, om = models(name)
    raw = whole("en" if "_en" in name else "de", name.partition(":")[0], om)[0]
    exp = {mode: om.transduce(raw, mode) for mode in MODES}
    assert all(e[1] == 0 for e in exp.values())
    for depth in (3, 2):
        with datok_amd.Stream(S, depth=depth) as st:
            for mode in MODES:
                slices = assert_rendered(st, tok, om, raw, mode, read_size=5000, exp=exp[mode][0])
                assert len(slices) >= 12
                assert om.transduce(raw, mode | NL)[0] == exp[mode][0]
                assert st.transduce(tok, raw, mode) == (exp[mode][0], 0), mode
                assert st.transduce(tok, raw, mode | NL) == (exp[mode][0], 0), mode


# ---- 2. every alignment of a cut
CUT_CASES = ([(c, n) for c in sc.CONSTRUCTS for n in ("tokenizer_de.matok", "tokenizer_de.datok")]
             + [(c, "tokenizer_de.matok:entries") for c in ("token300", "token4000")])


@pytest.mark.parametrize("construct,name", CUT_CASES)
def test_cut_alignment(models, name, construct):
    """(Over 16-bit entries: the two long tokens, at three shifts.)"""
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for shift in ((0, 1, 2, 3, 39) if ":entries" not in name else (0, 1, 39)):
            raw = sc.construct_stream(construct, shift)
            slices = assert_rendered(st, tok, om, raw, 3)
            if construct == "token5000":
                assert slices[-1].status & sc.ST_WINDOW_OVERFLOW
            elif construct == "token4000":
                assert any(int(e) - int(b) == 4000 for sl in slices for b, e in zip(sl.tok_bstart, sl.tok_bend))
        assert_rendered(st, tok, om, sc.construct_stream(construct, 1), 1)


# ---- 3. counts at the kernels' edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4096])
def test_token_counts_at_the_tile_edges(models, n):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b"a " * n
    with datok_amd.Stream(S) as st:
        for mode in (3, 1, 2, 0):
            slices = assert_rendered(st, tok, om, raw, mode)
            assert len(slices) == 1 and len(slices[0].tok_bend) == n


@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_dense_tokens_blanks_and_the_empty_stream(models, name):
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        raw = b"a b. " * 8000                  # two slices, dense tokens: several scan tiles, token arrays that regrow
        for mode in MODES:
            slices = assert_rendered(st, tok, om, raw, mode)
            assert len(slices) == 2 and len(slices[0].tok_bend) > 6000
        raw = b"Es geht so. " * 3400           # a SEPS entry on the cursor of every sentence's last END
        for mode in MODES:
            slices = assert_rendered(st, tok, om, raw, mode)
        sl = slices[0]
        assert len(sl.evl_pos) > 1000 and np.isin(sl.evl_pos[(sl.evl_kind & 4) != 0], sl.tok_bend).all()
        for raw in (b" " * 1000, b""):         # blanks only (fewer than a window holds), and the empty stream
            for mode in MODES:
                slices = assert_rendered(st, tok, om, raw, mode)
                assert len(slices) == 1 and len(slices[0].tok_bend) == 0


# ---- 4. bytes that do not decode
def _sow_invalid(text, leads=(0xC3,)):
    """`text` with \\xff, a lead byte + blank (`leads` in turn) and a truncated \\xe2\\x82 sown into tokens every 97 bytes;
    an \\xff as the last byte in front of every window's byte S."""
    b = bytearray(text)
    n = len(b)

    def letter(i):
        return 0x61 <= b[i] <= 0x7A
    for k, i in enumerate(range(97, n - 8, 97)):
        j = i
        if k % 3 == 1:
            while j < n - 4 and not (letter(j) and letter(j - 1) and b[j + 1] == 0x20):
                j += 1
            if j < n - 4:
                b[j] = leads[(k // 3) % len(leads)]
        else:
            while j < n - 4 and not (letter(j) and letter(j + 1) and letter(j + 2)):
                j += 1
            if j < n - 4:
                if k % 3 == 0:
                    b[j] = 0xFF
                else:
                    b[j], b[j + 1] = 0xE2, 0x82
    for w in range(1, 5):            # "... xy\xff " with the \xff at window byte S - 1
        at = w * S
        b[at - 4:at + 1] = b" xy\xff "
    return bytes(b)


_invalid = {}


def invalid_stream():
    """Running text with \\xff, \\xc3 + blank and a truncated \\xe2\\x82 sown into tokens every 97 bytes; an \\xff as the last
    byte in front of every window's byte S."""
    if "plain" not in _invalid:
        _invalid["plain"] = _sow_invalid(sc.running_text(5 * S, seed=21).replace(b"\x04", b" "))
    return _invalid["plain"]


def invalid_stream_spliced():
    """The same text with the characters of the enlarged model spliced in (bigsigma.splice) before the same bytes are sown
    by the same rule; every second lead byte in front of a blank is \\xd0, the lead byte of the new alphabet, left without
    its continuation.  For "de64.matok"."""
    if "spliced" not in _invalid:
        text = sc.running_text(5 * S, seed=21).replace(b"\x04", b" ")
        _invalid["spliced"] = _sow_invalid(bigsigma.splice(text, np.random.default_rng(7), limit=5 * S), leads=(0xC3, 0xD0))
    return _invalid["spliced"]


# the models of the tests of invalid bytes, here and in the three modules beside this one: codes; the same two automata
# over 16-bit entries; a model that has such a stream by itself, on the stream that holds its characters
INVALID_MODELS = ["tokenizer_de.matok", "tokenizer_de.matok:entries", "tokenizer_de.datok:entries", "de64.matok"]


def invalid_stream_of(name):
    return invalid_stream_spliced() if name == "de64.matok" else invalid_stream()


def code_twin(models, name):
    """The device model of the same file over a stream of codes, for an ":entries" name; else None.  Skips where the
    suite runs whole under the switch that gives every model 16-bit entries (bigsigma.has_code_twin)."""
    if ":entries" not in name:
        return None
    if not bigsigma.has_code_twin():
        pytest.skip("DATOK_SYM16 is set: no load in this process gives the stream of codes to compare with")
    return models(name.partition(":")[0])[0]


@pytest.mark.parametrize("name", INVALID_MODELS)
def test_invalid_utf8_prints_as_replacement_runes(models, name):
    import datok_amd
    tok, om = models(name)
    raw = invalid_stream_of(name)
    exp, est = om.transduce(raw, 3)
    assert est == 0 and exp.count(FFFD) >= 100 and raw.count(FFFD) == 0
    with datok_amd.Stream(S) as st:
        slices = assert_rendered(st, tok, om, raw, 3, exp=exp)
        ones = assert_rendered(st, tok, om, raw, 1)
    assert len(slices) == 5 if name != "de64.matok" else len(slices) >= 4
    assert sum(sl.out.count(FFFD) for sl in slices) == exp.count(FFFD)
    # one as the last byte in front of a cut, and one in a wave's 64th token
    assert any(not sl.last and sl.cut == S and sl.text[S - 1] == 0xFF for sl in slices)
    bad = set(b"\xff\xc3\xd0\xe2\x82")
    assert any(k % 64 == 63 and bad & set(sl.text[int(a):int(z)])
               for sl in slices for k, (a, z) in enumerate(zip(sl.tok_bstart, sl.tok_bend)))
    twin = code_twin(models, name)
    if twin is not None:          # the same automaton and the same stream: any difference is the stream format's
        with datok_amd.Stream(S) as st:
            for mode, mine in ((3, slices), (1, ones)):
                assert [sl.out for sl in assert_rendered(st, twin, om, raw, mode)] == [sl.out for sl in mine], mode


# ---- 5. later work on a slice
@pytest.mark.parametrize("chunk,warm", [(16, 0), (0, 8)])
def test_repair_rounds_and_one_lane_per_slice(models, whole, chunk, warm):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    with datok_amd.Stream(S) as st:
        st.set_chunking(chunk, warm)
        assert_rendered(st, tok, om, raw, 3)


def test_a_list_packed_twice_is_rendered_twice(models, whole):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    with datok_amd.Stream(S) as st:
        assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"1") == 0
        try:
            slices = assert_rendered(st, tok, om, raw, 3)
        finally:
            assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", os.environ.get("DATOK_EVL_CAP", "-1").encode()) == 0
        assert sum(len(sl.evl_pos) > 1 for sl in slices) >= 10


# ---- 6. reuse
def test_one_stream_object_through_modes(models, whole):
    import datok_amd
    from datok_amd import _lib
    tok, om = models("tokenizer_de.matok")
    raw, calls, ost = whole("de", "tokenizer_de.matok", om)
    with datok_amd.Stream(S) as st:
        assert_rendered(st, tok, om, raw, 3)
        st.set_render(None)
        slices, status = run_rendered(st, tok, raw)
        assert all(sl.out is None for sl in slices)
        assert sc.stream_calls(True, slices) == calls and status == ost
        assert_rendered(st, tok, om, raw, 1)
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_render(1 | 4)
        assert e.value.code == _lib.E_ARG
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_render(8)
        assert e.value.code == _lib.E_ARG
        assert_rendered(st, tok, om, sc.running_text(30000, seed=2), 1)       # (still mode 1, a shorter stream)
        assert_rendered(st, tok, om, sc.running_text(30000, seed=2), 2)
        # a position mode of the mirror turns rendering off and replays
        assert st.transduce(tok, raw, 15) == om.transduce(raw, 15)
        slices, _ = run_rendered(st, tok, raw)
        assert all(sl.out is None for sl in slices)


# ---- 7. the command line
@pytest.mark.parametrize("flags,mode", [((), 3), (("--no-tokens",), 2), (("--no-sentences",), 1), (("--token-positions",), 7)])
def test_cli_writes_the_rendered_bytes(tmp_path, flags, mode):
    from oracle import oracle as O
    om = O.Model(os.path.join(MODELS, "tokenizer_de.matok"))
    raw = sc.running_text(300 * 1024, seed=12)
    exp, st = om.transduce(raw, mode)
    assert st == 0
    f = tmp_path / "in.txt"
    f.write_bytes(raw)
    cli = os.path.join(ROOT, "datok_amd", "datok")
    cmd = [cli, "tokenize", "-t", os.path.join(MODELS, "tokenizer_de.matok"), "--slice-bytes", "16384"] + list(flags)
    out = subprocess.run(cmd + [str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == exp
    out = subprocess.run(cmd + ["-"], input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == exp
