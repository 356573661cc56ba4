"""The position renderer's specification without a GPU: streampos.render_slice_pos_ref -- the writer's rules on one
slice's calls with the state carried in, as dtk_streampos.hip computes them -- and streampos.emit_ref, the splice of
dtk_stream_emit, on synthetic slice views cut from the oracle's calls.  The emitted bytes of all slices are the oracle's
bytes for the whole stream and what the Python replay writes into one stock writer, in the 12 modes with TOKEN_POS or
SENTENCE_POS, each with and without NEWLINE_AFTER_EOT; every slice's carry_out is the writer's state behind it."""
import io

import numpy as np
import pytest

import streamcorpus as sc
from streampos import CARRY0, emit_ref, mirror_token_writer, render_slice_pos_ref

POS_MODES = [m for m in range(16) if m & 12]
MODELS = ["tokenizer_de.matok", "tokenizer_de.datok"]
NL = 16


def _check(om, raw, empty_text=False):
    from datok_amd import host
    is_matrix = om.type() == "MATOK"
    calls, st = sc.oracle_calls(om, raw)
    assert st == (sc.ST_EMPTY_TEXT if empty_text else 0) or raw.count(b"a" * 5000)
    slices = sc.synthetic_slices(is_matrix, raw, calls, sc.S)
    assert len(slices) >= 2
    for nl in (0, NL):
        for mode in POS_MODES:
            bits = mode | nl
            held, carry, got = [bytearray(), bytearray()], CARRY0, bytearray()
            w = io.BytesIO()
            tw, state = mirror_token_writer(w, bits)
            for i, sl in enumerate(slices):
                r = render_slice_pos_ref(is_matrix, sl, bits, carry)
                got += emit_ref(held, r)
                host.replay_slice(is_matrix, sl, tw)
                carry = r[5]
                assert carry == (state["posC"], state["sentB"], state["init"], bool(state["pos"]), bool(state["sent"])), (bits, i)
                # what is held is the open text's line so far
                if bits & host.TOKEN_POS:
                    assert bytes(held[0]) == " ".join(map(str, state["pos"])).encode(), (bits, i)
                if bits & host.SENTENCE_POS:
                    assert bytes(held[1]) == " ".join(map(str, state["sent"])).encode(), (bits, i)
            assert bytes(got) == w.getvalue(), bits
            if not empty_text:
                w2 = io.BytesIO()
                tw2 = host.new_token_writer(w2, bits)
                for sl in slices:
                    host.replay_slice(is_matrix, sl, tw2)
                tw2.Flush()
                assert bytes(got) == w2.getvalue(), bits
                assert bytes(got) == om.transduce(raw, bits)[0], bits


@pytest.mark.parametrize("model", MODELS)
def test_reference_renders_the_200k_stream(oracle_models, model):
    om = oracle_models(model)
    raw = sc.running_text(200 * 1024, seed=5)
    assert raw.count(b"\x04") >= 10
    _check(om, raw)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("construct", list(sc.CONSTRUCTS))
def test_reference_renders_every_construct(oracle_models, model, construct):
    om = oracle_models(model)
    for shift in (0, 1, 39):
        _check(om, sc.construct_stream(construct, shift))


def empty_text_streams():
    """The stream shapes of test_stream.py's test_empty_text_is_decided_across_cuts: (stream, has an empty text)."""
    fill = sc.running_text(3 * sc.S, seed=4).replace(b"\x04", b" ")
    for shift in range(0, 24, 3):
        left = fill[:sc.S - 12 + shift]
        left = left[:left.rfind(b" ")] + b". "
        yield left + b" " * 40 + b"\x04\nWeiter geht es. " + fill[:sc.S], False
        for extra in (b" " * 40 + b"\x04 \x04\nWeiter. ", b"\x04" + b" " * 40 + b"\x04\nWeiter. "):
            yield left + extra + fill[:sc.S], True


@pytest.mark.parametrize("model", MODELS)
def test_reference_prints_empty_texts_as_the_mirror_does(oracle_models, model):
    om = oracle_models(model)
    for raw, empty in empty_text_streams():
        _check(om, raw, empty_text=empty)


def test_a_text_end_right_behind_the_cut():
    """One slice by hand: the TextEnd of a text that began earlier fires before any token of this slice, so its lines
    hold none of this slice's position integers -- the held prefix and a newline -- and one sentence integer."""
    from datok_amd import host
    text = b"x.\x04\nab c"
    sl = host.SliceView(base=16384, first=2, cut=len(text), last=1, status=0, text=text,
                        tok_bstart=np.array([4, 7], np.uint32), tok_bend=np.array([6, 8], np.uint32),
                        evl_pos=np.array([3], np.uint32), evl_kind=np.array([host.EVL_SEOT | host.EVL_TEOT], np.uint8),
                        tail=len(text) << 2 | 3)
    carry = (7, False, False, True, True)
    r = render_slice_pos_ref(True, sl, 15, carry)
    assert r == (b"\n" b"\n" b" 7\n" b"ab\nc\n" b"\n" b"1 3 4 5\n" b"1 5\n", 1, 2, b"", b"", (0, True, False, False, False))
    held = [bytearray(b"0 1 2 7"), bytearray(b"0")]
    assert emit_ref(held, r) == b"\n0 1 2 7\n0 7\nab\nc\n\n1 3 4 5\n1 5\n" and held == [b"", b""]
    # the newline rule at the slice's first token: posC is 0 behind the TextEnd, the window starts with '\n'
    r = render_slice_pos_ref(True, sl, 31, carry)
    assert r[0] == b"\n\n 7\nab\nc\n\n0 2 3 4\n0 4\n" and r[1:3] == (1, 2)
    # TOKEN_POS alone: no sentence line, and the text stays open without the tail
    sl.last, sl.tail = 0, 0
    r = render_slice_pos_ref(True, sl, 5, carry)
    assert r == (b"\nab\nc\n", 0, None, b"1 3 4 5", b"", (5, False, False, True, True))
    held = [bytearray(b"0 1 2 7"), bytearray()]
    assert emit_ref(held, r) == b"0 1 2 7\nab\nc\n" and held == [b"1 3 4 5", b""]
    # a second slice of the same text: its integers follow a blank
    r = render_slice_pos_ref(True, host.SliceView(base=0, first=0, cut=3, last=0, status=0, text=b" de",
                                                  tok_bstart=np.array([1], np.uint32), tok_bend=np.array([3], np.uint32),
                                                  evl_pos=np.zeros(0, np.uint32), evl_kind=np.zeros(0, np.uint8)), 12, r[5])
    assert r == (b"", None, None, b" 6 8", b"", (8, False, False, True, True))


def test_set_position_render_checks_its_arguments():
    import ctypes as C
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    for name in ("dtk_stream_set_position_render", "dtk_stream_positions", "dtk_stream_emit"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    for bits in (0, 3, 4, 15, 31, 32):
        assert L.dtk_stream_set_position_render(None, 1, bits) == _lib.E_ARG
    assert L.dtk_stream_set_position_render(None, 0, 0) == _lib.E_ARG
    assert L.dtk_stream_positions(None, None) == _lib.E_ARG
    assert L.dtk_stream_emit(None, _lib.WRITE_FN(lambda u, p, n: 0), None) == _lib.E_ARG
    # dtk_stream_slice keeps its layout
    assert [f for f, _ in _lib.StreamSlice._fields_][-2:] == ["out", "out_len"]
    assert C.sizeof(_lib.StreamCarry) == 24 and C.sizeof(_lib.StreamPos) == 48 + 2 * 24
    h = C.c_void_p()
    if L.dtk_device_count() > 0:
        assert L.dtk_stream_create(16384, 3, C.byref(h)) == _lib.OK
        for bits in (4, 8, 12, 15, 31, 20):
            assert L.dtk_stream_set_position_render(h, 1, bits) == _lib.OK
        for bits in (0, 1, 3, 16, 19, 32, 36, 1 << 31):
            assert L.dtk_stream_set_position_render(h, 1, bits) == _lib.E_ARG
        assert L.dtk_stream_set_position_render(h, 0, 0) == _lib.OK
        sp = _lib.StreamPos()
        assert L.dtk_stream_positions(h, C.byref(sp)) == _lib.E_STATE      # (outside slice_fn)
        L.dtk_stream_free(h)


def test_every_export_is_in_the_library():
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    missing = [n for n in _lib.EXPORTS if not hasattr(L, n)]
    assert not missing
    header = open(datok_amd.__file__.replace("datok_amd/__init__.py", "include/datok_gpu.h")).read()
    assert all(n + "(" in header for n in _lib.EXPORTS if n.startswith("dtk_stream"))


def test_a_trailer_that_is_not_regular_ends_the_run():
    """The block that comes home behind a slice's bytes (DtkPosTrailer, dtk_internal.h) decides whether the bytes are
    delivered: a length beyond the capacity, a list that did not fit its arrays (out_len = ~0) or a tile whose integers
    pass 2^32 bytes are DTK_E_CAPACITY; a token with rend == 0 under NEWLINE_AFTER_EOT, where the literal rule would fire
    a second time, is DTK_E_IRREGULAR -- never a silently different number."""
    import ctypes as C
    import datok_amd
    from datok_amd import _lib

    class Trailer(C.Structure):
        _fields_ = [("out_len", C.c_uint64), ("open_pos_len", C.c_uint64), ("open_sent_len", C.c_uint64),
                    ("splice_pos", C.c_uint64), ("splice_sent", C.c_uint64), ("carry_in", _lib.StreamCarry),
                    ("carry_out", _lib.StreamCarry), ("flags", C.c_uint32), ("pad", C.c_uint32)]
    assert C.sizeof(Trailer) == 40 + 2 * 24 + 8
    check = datok_amd.lib().dtk_pos_trailer_check
    check.argtypes = [C.POINTER(Trailer), C.c_uint64]

    def rc(cap=100, **kw):
        t = Trailer(**{"out_len": 60, "open_pos_len": 30, "open_sent_len": 10, **kw})
        return check(C.byref(t), cap)
    assert rc() == _lib.OK
    assert rc(cap=99) == _lib.E_CAPACITY
    assert rc(out_len=2 ** 64 - 1) == _lib.E_CAPACITY
    assert rc(out_len=61) == _lib.E_CAPACITY
    assert rc(open_pos_len=2 ** 64 - 40) == _lib.E_CAPACITY            # (no sum that wraps)
    assert rc(open_sent_len=2 ** 64 - 80) == _lib.E_CAPACITY
    assert rc(flags=2) == _lib.E_CAPACITY
    assert rc(flags=1) == _lib.E_IRREGULAR
    assert rc(flags=3) == _lib.E_CAPACITY
    assert check(None, 100) == _lib.E_ARG
