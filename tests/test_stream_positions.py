"""A stream's position modes rendered on the device (dtk_stream_set_position_render, dtk_streampos.hip): with TOKEN_POS or
SENTENCE_POS the writer's state is carried from slice to slice on the device, and dtk_stream_emit puts a text's position
lines together across cuts.  Every test compares each slice's six outputs with streampos.render_slice_pos_ref of that
slice's own arrays and carry_in, so that a failure names the slice, and the emitted bytes of all slices with the
oracle's bytes for the WHOLE stream."""
import io
import os
import subprocess

import pytest

import streamcorpus as sc
from conftest import MODELS, ROOT
from streampos import CARRY0, emit_ref, mirror_token_writer, render_slice_pos_ref
from test_stream import models, whole  # noqa: F401  (fixtures: the device and oracle models, the 200 KB streams)
from test_stream_positions_host import empty_text_streams
from test_stream_render import INVALID_MODELS, code_twin, invalid_stream_of

pytestmark = pytest.mark.gpu

S = sc.S
POS_MODES = [m for m in range(16) if m & 12]
NL = 16
SIX = ("out", "splice_pos", "splice_sent", "open_pos", "open_sent", "carry_out")


def run_positions(st, tok, raw, bits, read_size=None):
    r = io.BytesIO(raw)
    if read_size:
        class Short:
            def read(self, n):
                return r.read(min(n, read_size))
        reader = Short()
    else:
        reader = r
    slices = []
    status = st.run(tok, reader, flags=bits & NL, on_slice=slices.append)
    return slices, status


def oracle_prefix(om, raw, bits):
    """Bytes the writer has written when the reference's window overflows: the oracle's calls in front of the token
    that fits no window (test_stream.py, assert_stream), replayed into a stock writer."""
    from datok_amd import host
    calls = sc.oracle_calls(om, raw)[0]
    n = next(i for i, c in enumerate(calls) if c[0] == 0 and c[4] - c[2] > 4104)
    assert n > 100
    w = io.BytesIO()
    tw = host.new_token_writer(w, bits)
    for c in calls[:n]:
        if c[0] == 0:
            tw.Token(c[1], host._decode_runes(raw[c[2]:c[4]]))
        else:
            (tw.SentenceEnd if c[0] == 1 else tw.TextEnd)(c[1])
    tw.Flush()
    return len(w.getvalue())


def mirror_bytes(st, tok, raw, bits):
    """What the C++ mirror's writer writes for the stream: its rules in Python, fed by the replay of a plain run."""
    from datok_amd import host
    st.set_render(None)
    st.set_position_render(None)
    plain, _ = run_positions(st, tok, raw, 0)
    w = io.BytesIO()
    tw, _ = mirror_token_writer(w, bits)
    for sl in plain:
        host.replay_slice(tok.type() == "MATOK", sl, tw)
    return w.getvalue()


def assert_positions(st, tok, om, raw, bits, read_size=None, exp=None, carry0=CARRY0, held_peak=None):
    """Renders `raw` in the position mode `bits` on `st`; returns the slices."""
    is_matrix = tok.type() == "MATOK"
    st.set_position_render(bits)
    slices, status = run_positions(st, tok, raw, bits, read_size)
    sc.check_slices(slices, len(raw))
    held, carry = [bytearray(), bytearray()], carry0
    for i, sl in enumerate(slices):
        assert sl.out is not None and sl.carry_in == carry, (i, sl.carry_in, carry)
        ref = render_slice_pos_ref(is_matrix, sl, bits, sl.carry_in)
        for name, want in zip(SIX, ref):
            got = getattr(sl, name)
            if got != want:
                k = (next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
                     if isinstance(got, bytes) and isinstance(want, bytes) else 0)
                raise AssertionError("slice %d of %d (base %d, %d tokens, %d entries, carry_in %r), mode %d, %s: %r against %r"
                                     % (i, len(slices), sl.base, len(sl.tok_bend), len(sl.evl_pos), sl.carry_in, bits, name,
                                        got[max(k - 30, 0):k + 30] if isinstance(got, bytes) else got,
                                        want[max(k - 30, 0):k + 30] if isinstance(want, bytes) else want))
        assert sl.written == emit_ref(held, ref), (bits, i)
        if held_peak is not None:
            held_peak.append(len(held[0]))
        carry = sl.carry_out
    got = b"".join(sl.written for sl in slices)
    if exp is None:
        exp = om.transduce(raw, bits)[0]
    if status & sc.ST_WINDOW_OVERFLOW:
        k = oracle_prefix(om, raw, bits)
        assert len(got) >= k
        got, exp = got[:k], exp[:k]
    assert len(got) == len(exp), (bits, len(got), len(exp))
    assert got == exp, bits
    return slices


MODELS_1 = ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_de.datok:pairs", "tokenizer_en.matok"]


# ---- 1. the 200 KB streams
@pytest.mark.parametrize("name", MODELS_1)
def test_position_modes_equal_the_oracles_bytes(models, whole, name):
    import datok_amd
    tok, om = models(name)
    raw = whole("en" if "_en" in name else "de", name.partition(":")[0], om)[0]
    exp = {mode | nl: om.transduce(raw, mode | nl) for mode in POS_MODES for nl in (0, NL)}
    assert all(e[1] == 0 for e in exp.values())
    for depth in (3, 2):
        with datok_amd.Stream(S, depth=depth) as st:
            for bits in exp:
                slices = assert_positions(st, tok, om, raw, bits, read_size=5000, exp=exp[bits][0])
                assert len(slices) >= 12
                assert st.transduce(tok, raw, bits) == (exp[bits][0], 0), bits


# ---- 2. every alignment of a cut
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
@pytest.mark.parametrize("construct", list(sc.CONSTRUCTS))
def test_cut_alignment(models, name, construct):
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for shift in (0, 1, 2, 3, 39):
            raw = sc.construct_stream(construct, shift)
            assert construct == "token5000" or sc.oracle_calls(om, raw)[1] == 0
            for bits in (15, 31, 4, 8, 13):
                slices = assert_positions(st, tok, om, raw, bits)
            if construct == "token5000":
                assert slices[-1].status & sc.ST_WINDOW_OVERFLOW
            elif construct == "token4000":
                assert any(int(e) - int(b) == 4000 for sl in slices for b, e in zip(sl.tok_bstart, sl.tok_bend))


# ---- 3. a text that spans five slices
def test_a_text_of_five_slices(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = sc.running_text(5 * S, seed=21).replace(b"\x04", b" ")
    assert om.transduce(raw, 15)[1] == 0
    with datok_amd.Stream(S) as st:
        for bits in (15, 31, 4):
            peak = []
            slices = assert_positions(st, tok, om, raw, bits, held_peak=peak)
            assert len(slices) == 5
            assert all(sl.open_pos and sl.splice_pos is None for sl in slices[:-1]) and not slices[-1].open_pos
            assert slices[-1].splice_pos is not None
            assert max(peak) > 4 * S * 0.1


# ---- 4. decimal lengths
def test_decimal_lengths_within_and_across_slices(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b"a " * 60000
    assert om.transduce(raw, 12)[1] == 0
    with datok_amd.Stream(S) as st:
        for bits in (12, 15, 28):
            slices = assert_positions(st, tok, om, raw, bits)
            assert len(slices) >= 7 and b" 99999 100000 " in b"".join(sl.written for sl in slices)


def test_positions_beyond_32_bits(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b"a " * 200
    base = 9999999950
    exp, est = om.transduce(raw, 12)
    assert est == 0
    lines = exp.split(b"\n")
    assert len(lines) == 3 and lines[2] == b""
    want = b"".join(b" ".join(str(int(x) + base).encode() for x in ln.split()) + b"\n" for ln in lines[:2])
    assert b" 9999999999 10000000000 " in want and int(want.split()[0]) > 2 ** 32
    L = datok_amd.lib()
    with datok_amd.Stream(S) as st:
        assert L.dtk_debug_configure(b"SP_POSC0", str(base).encode()) == 0
        try:
            slices = assert_positions(st, tok, om, raw, 12, exp=want, carry0=(base, True, True, False, False))
        finally:
            assert L.dtk_debug_configure(b"SP_POSC0", b"0") == 0
        assert len(slices) == 1
        assert_positions(st, tok, om, raw, 12, exp=exp)           # (the key is read at a run's start: off again)


# ---- 5. counts at the kernels' edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096])
def test_token_counts_at_the_tile_edges(models, n):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b"a " * n
    assert om.transduce(raw, 15)[1] == (0 if n else sc.ST_EMPTY_TEXT)
    with datok_amd.Stream(S) as st:
        for bits in (15, 4):
            # (the empty stream is an empty text: the reference panics, the mirror prints no line)
            slices = assert_positions(st, tok, om, raw, bits, exp=None if n else mirror_bytes(st, tok, raw, bits))
            assert len(slices) == 1 and len(slices[0].tok_bend) == n


@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_dense_sentences_blanks_and_the_empty_stream(models, name):
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for raw in (b"a b. " * 8000, b"Es geht so. " * 3400):   # a sentence integer at almost every token
            assert om.transduce(raw, 15)[1] == 0
            for bits in (15, 31, 8, 4):
                slices = assert_positions(st, tok, om, raw, bits)
            assert len(slices) >= 2 and len(slices[0].tok_bend) > 4000
        assert len(slices[0].evl_pos) > 1000
        for raw in (b" " * 1000, b""):                           # no token at all: the mirror prints no line
            for bits in (15, 4):
                slices = assert_positions(st, tok, om, raw, bits, exp=mirror_bytes(st, tok, raw, bits))
                assert len(slices) == 1 and len(slices[0].tok_bend) == 0


# ---- 6. bytes that do not decode
@pytest.mark.parametrize("name", INVALID_MODELS)
def test_invalid_utf8_counts_as_one_rune_a_byte(models, name):
    import datok_amd
    tok, om = models(name)
    raw = invalid_stream_of(name)
    assert om.transduce(raw, 15)[1] == 0
    mine = {}
    with datok_amd.Stream(S) as st:
        for bits in (7, 15):
            slices = mine[bits] = assert_positions(st, tok, om, raw, bits)
        assert len(slices) == 5 if name != "de64.matok" else len(slices) >= 4
        assert sum(sl.out.count(b"\xef\xbf\xbd") for sl in slices) >= 100
    twin = code_twin(models, name)
    if twin is not None:          # the same automaton and the same stream: any difference is the stream format's
        with datok_amd.Stream(S) as st:
            for bits in (7, 15):
                theirs = assert_positions(st, twin, om, raw, bits)
                assert [(sl.out, sl.written, sl.carry_out) for sl in theirs] == [(sl.out, sl.written, sl.carry_out) for sl in mine[bits]]


# ---- 7. later work on a slice
@pytest.mark.parametrize("chunk,warm", [(16, 0), (0, 8)])
def test_repair_rounds_and_one_lane_per_slice(models, whole, chunk, warm):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    with datok_amd.Stream(S) as st:
        st.set_chunking(chunk, warm)
        assert_positions(st, tok, om, raw, 15)


def test_a_slice_rendered_twice_leaves_the_same_carry(models, whole):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    with datok_amd.Stream(S) as st:
        plain = assert_positions(st, tok, om, raw, 15)
        assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"1") == 0
        try:
            slices = assert_positions(st, tok, om, raw, 15)
        finally:
            assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", os.environ.get("DATOK_EVL_CAP", "-1").encode()) == 0
        assert sum(len(sl.evl_pos) > 1 for sl in slices) >= 10
        assert [sl.carry_out for sl in slices] == [sl.carry_out for sl in plain]


# ---- 8. empty texts
def test_empty_texts_print_as_the_mirror_does(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    with datok_amd.Stream(S) as st:
        for k, (raw, empty) in enumerate(empty_text_streams()):
            ost = sc.oracle_calls(om, raw)[1]
            assert ost == (sc.ST_EMPTY_TEXT if empty else 0)
            exp = mirror_bytes(st, tok, raw, 15)
            slices = assert_positions(st, tok, om, raw, 15, exp=exp)
            status = 0
            for sl in slices:
                status |= sl.status
            assert status & sc.ST_EMPTY_TEXT == ost & sc.ST_EMPTY_TEXT
            if not empty:
                assert exp == om.transduce(raw, 15)[0]


# ---- 9. reuse
def test_one_stream_object_through_modes(models, whole):
    import datok_amd
    from datok_amd import _lib
    from test_stream_render import assert_rendered
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    short = sc.running_text(30000, seed=2)
    with datok_amd.Stream(S) as st:
        assert_positions(st, tok, om, raw, 15)
        with pytest.raises(_lib.DatokGpuError) as e:      # the run's flags must carry the rendering's newline bit
            st.run(tok, raw, flags=NL)
        assert e.value.code == _lib.E_ARG
        assert_rendered(st, tok, om, raw, 3)              # set_render turns position rendering off: plain bytes
        assert all(sl.written is None and sl.carry_out is None for sl in assert_rendered(st, tok, om, short, 3))
        st.set_render(None)
        slices, _ = run_positions(st, tok, raw, 0)
        assert all(sl.out is None and sl.written is None for sl in slices)
        assert_positions(st, tok, om, short, 15)          # a shorter stream: the carry and what is held start fresh
        assert_positions(st, tok, om, short, 28)
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_render(7)
        assert e.value.code == _lib.E_ARG
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_position_render(3)
        assert e.value.code == _lib.E_ARG
        assert_positions(st, tok, om, short, 28)          # (a refused call changes nothing)
        assert st.transduce(tok, raw, 15) == om.transduce(raw, 15)
        slices, _ = run_positions(st, tok, raw, 0)        # dtk_stream_transduce leaves both renderers off
        assert all(sl.out is None for sl in slices)


# ---- 10. the command line
def test_cli_writes_position_lines(tmp_path):
    from oracle import oracle as O
    om = O.Model(os.path.join(MODELS, "tokenizer_de.matok"))
    raw = sc.running_text(300 * 1024, seed=12)
    exp, st = om.transduce(raw, 31)
    assert st == 0
    f = tmp_path / "in.txt"
    f.write_bytes(raw)
    cli = os.path.join(ROOT, "datok_amd", "datok")
    cmd = [cli, "tokenize", "-t", os.path.join(MODELS, "tokenizer_de.matok"), "--slice-bytes", "16384",
           "--token-positions", "--sentence-positions", "--newline-after-eot"]
    out = subprocess.run(cmd + [str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == exp
    out = subprocess.run(cmd + ["-"], input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == exp
