"""The stream renderer's specification without a GPU: streamrender.render_slice_ref -- the merge of a slice's tokens
with its event list and the size of every piece, as dtk_streamrender.hip computes them -- on synthetic slice views cut
from the oracle's calls.  The slices' bytes, one after the other, are the oracle's bytes for the whole stream and what
the Python replay writes into one stock writer, in the four position-free modes with and without NEWLINE_AFTER_EOT."""
import io

import pytest

import streamcorpus as sc
from streamrender import render_slice_ref

MODES = (0, 1, 2, 3)
MODELS = ["tokenizer_de.matok", "tokenizer_de.datok"]


def _check(om, raw):
    from datok_amd import host
    is_matrix = om.type() == "MATOK"
    calls, st = sc.oracle_calls(om, raw)
    # (the oracle walks on where the reference's window overflows -- token5000: its calls and bytes are compared whole)
    slices = sc.synthetic_slices(is_matrix, raw, calls, sc.S)
    assert len(slices) >= 2
    for nl in (0, host.NEWLINE_AFTER_EOT):
        for mode in MODES:
            got = b"".join(render_slice_ref(is_matrix, sl, mode | nl) for sl in slices)
            w = io.BytesIO()
            tw = host.new_token_writer(w, mode | nl)
            for sl in slices:
                host.replay_slice(is_matrix, sl, tw)
            tw.Flush()
            assert got == w.getvalue(), (mode, nl)
            assert got == om.transduce(raw, mode | nl)[0], (mode, nl)


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


def test_reference_expands_bytes_that_do_not_decode(oracle_models):
    """One slice by hand: a token with an invalid byte is two bytes longer, and SEOT, TEOT stand in front of a token on
    their cursor, SEPS behind it."""
    import numpy as np
    from datok_amd import host
    text = b"ab\xffc d.\x04e"
    sl = host.SliceView(base=0, first=0, cut=len(text), last=1, status=0, text=text,
                        tok_bstart=np.array([0, 5, 6, 8], np.uint32), tok_bend=np.array([4, 6, 7, 9], np.uint32),
                        evl_pos=np.array([7, 8], np.uint32),
                        evl_kind=np.array([host.EVL_SEPS, host.EVL_SEOT | host.EVL_TEOT], np.uint8), tail=9 << 2 | 3)
    assert render_slice_ref(True, sl, 3) == b"ab\xef\xbf\xbdc\nd\n.\n\n\n\ne\n\n\n"
    assert render_slice_ref(True, sl, 1) == b"ab\xef\xbf\xbdc\nd\n.\n\ne\n\n"
    assert render_slice_ref(True, sl, 2) == b"\n\n\n\n\n"
    assert render_slice_ref(True, sl, 0) == b"\n\n"
    w = io.BytesIO()
    tw = host.new_token_writer(w, 3)
    host.replay_slice(True, sl, tw)
    tw.Flush()
    assert w.getvalue() == render_slice_ref(True, sl, 3)


def test_set_render_checks_its_arguments():
    import ctypes as C
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    assert "dtk_stream_set_render" in _lib.EXPORTS
    assert L.dtk_stream_set_render(None, 1, 3) == _lib.E_ARG
    assert L.dtk_stream_set_render(None, 0, 0) == _lib.E_ARG
    names = [f for f, _ in _lib.StreamSlice._fields_]
    assert names[-2:] == ["out", "out_len"] and _lib.StreamSlice.out.offset == _lib.StreamSlice.view.offset + C.sizeof(_lib.ResultView)
    h = C.c_void_p()
    if L.dtk_device_count() > 0:
        assert L.dtk_stream_create(16384, 3, C.byref(h)) == _lib.OK
        for bits in (0, 1, 2, 3, 16, 19):
            assert L.dtk_stream_set_render(h, 1, bits) == _lib.OK
        for bits in (4, 8, 7, 32, 1 << 31):
            assert L.dtk_stream_set_render(h, 1, bits) == _lib.E_ARG
        L.dtk_stream_free(h)


def test_spliced_invalid_stream_is_what_its_tests_need():
    """test_stream_render.invalid_stream_spliced, the input of every "de64.matok" case of the stream tests, on the oracle
    of the enlarged model alone: in contract in the SIMPLE and in the position modes, with bytes that do not decode, the
    new characters, and places where one touches the other."""
    import bigsigma
    from datok_amd import host
    from streamrender import FFFD
    from test_stream_render import invalid_stream, invalid_stream_spliced
    raw = invalid_stream_spliced()
    assert raw is invalid_stream_spliced() and raw != invalid_stream()
    assert 5 * sc.S - 4 <= len(raw) <= 5 * sc.S and raw.count(FFFD) == 0
    om = bigsigma.oracle_of(bigsigma.enlarged_de(64))
    exp, status = om.transduce(raw, 3)
    assert status == 0 and om.transduce(raw, 15)[1] == 0
    assert exp.count(FFFD) >= 100
    runes = host._decode_runes(raw)                       # (no literal U+FFFD in it: every 0xFFFD here is a byte that does not decode)
    new = {ord(c) for c in bigsigma.CHARS}
    n_new = sum(r in new for r in runes)
    touching = sum(1 for i, r in enumerate(runes) if r in new and 0xFFFD in runes[max(i - 1, 0):i + 2])
    print("%d bytes, %d new characters, %d U+FFFD in the SIMPLE output, %d new characters beside a bad byte"
          % (len(raw), n_new, exp.count(FFFD), touching))
    assert n_new >= 1000 and touching >= 50
    assert any(raw[w * sc.S - 1] == 0xFF for w in range(1, 5))
    assert raw.count(b"\xd0 ") >= 20                      # the new alphabet's lead byte without its continuation
