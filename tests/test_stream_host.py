"""One stream in slices, host side (no GPU): the Python stream replay on synthetic slice views cut from the oracle's
calls, the corpora of tests/test_stream.py, and the new entry points' argument and device checks."""
import io
import os

import pytest

import streamcorpus as sc
from conftest import MODELS


def _text_60k():
    return sc.running_text(60 * 1024, seed=3, text_bytes=7000)


@pytest.mark.parametrize("model", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_synthetic_slices_replay_to_the_oracles_bytes(oracle_models, model):
    """The oracle's call list of a 60 KB stream with EOT texts, cut at rewinds into slice views (first, cut, tokens,
    entries), replayed slice by slice into ONE writer: the oracle's bytes for the whole stream, in all 16 writer
    modes, with and without NEWLINE_AFTER_EOT."""
    from datok_amd import host
    om = oracle_models(model)
    is_matrix = om.type() == "MATOK"
    whole = _text_60k()
    assert whole.count(b"\x04") >= 6
    calls, st = sc.oracle_calls(om, whole)
    assert st == 0
    slices = sc.synthetic_slices(is_matrix, whole, calls, sc.S)
    assert len(slices) >= 3
    sc.check_slices(slices, len(whole))
    assert sc.stream_calls(is_matrix, slices) == calls       # every call, in order, in stream bytes
    for nl in (0, host.NEWLINE_AFTER_EOT):
        for mode in sc.MODES:
            w = io.BytesIO()
            tw = host.new_token_writer(w, mode | nl)
            for sl in slices:
                host.replay_slice(is_matrix, sl, tw)
            tw.Flush()
            assert w.getvalue() == om.transduce(whole, mode | nl)[0], (mode, nl)


def test_a_cut_at_a_matrix_text_end_keeps_the_closing_calls(oracle_models):
    """A TextEnd fired by an EOT rewinds the matrix's window: a cut may lie there.  SentenceEnd and TextEnd at the cut
    are the slice's own; the next slice begins behind them."""
    from datok_amd import host
    om = oracle_models("tokenizer_de.matok")
    whole = b"Der erste Text endet hier.\x04\nDer zweite beginnt. " * 900
    whole = whole[:sc.S - 1] + b"\x04" + whole[sc.S:]                       # an EOT right in front of byte S
    calls, st = sc.oracle_calls(om, whole)
    slices = sc.synthetic_slices(True, whole, calls, sc.S)
    assert st == 0 and slices[0].cut == sc.S and slices[1].first == 0
    assert int(slices[0].evl_pos[-1]) == sc.S and int(slices[0].evl_kind[-1]) & host.EVL_TEOT
    assert sc.stream_calls(True, slices) == calls


@pytest.mark.parametrize("model", ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_en.matok"])
def test_the_gpu_tests_corpora_are_regular(oracle_models, model):
    """The oracle reports no status on the corpora of tests/test_stream.py, except the intended window overflow."""
    om = oracle_models(model)
    lang = "en" if "_en" in model else "de"
    assert om.events(sc.running_text(200 * 1024, seed=5, lang=lang))[1] == 0
    for name in sc.CONSTRUCTS:
        for shift in (0, 7, 40):
            st = om.events(sc.construct_stream(name, shift))[1]
            assert st == (sc.ST_WINDOW_OVERFLOW if name == "token5000" else 0), (name, shift, st)
    # the 4000-byte token is ONE token of 1000 runes
    raw = sc.construct_stream("token4000", 0)
    assert any(c[0] == 0 and c[4] - c[3] == 4000 for c in sc.oracle_calls(om, raw)[0])


def test_stream_symbols_and_argument_checks():
    import ctypes as C
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    for name in ("dtk_stream_create", "dtk_stream_free", "dtk_stream_set_chunking", "dtk_stream_set_result_fields",
                 "dtk_stream_run", "dtk_stream_transduce"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert _lib.E_IRREGULAR == -10
    msg = L.dtk_strerror(_lib.E_IRREGULAR).decode()
    assert "one document" in msg and msg != L.dtk_strerror(-99).decode()
    h = C.c_void_p()
    # bad arguments are refused before a device is looked for
    for slice_bytes, depth in ((0, 3), (16383, 3), (8192, 3), (16384 + 128, 3), (1 << 31, 3), (16384, 1), (16384, 17)):
        assert L.dtk_stream_create(slice_bytes, depth, C.byref(h)) == _lib.E_ARG, (slice_bytes, depth)
        assert not h.value
    assert L.dtk_stream_create(16384, 3, None) == _lib.E_ARG
    rc = L.dtk_stream_create(16384, 3, C.byref(h))
    if L.dtk_device_count() <= 0:
        assert rc == _lib.E_NO_DEVICE and not h.value
        with pytest.raises(_lib.DatokGpuError) as e:
            datok_amd.Stream(16384)
        assert e.value.code == _lib.E_NO_DEVICE
    else:
        assert rc == _lib.OK and h.value
        assert L.dtk_stream_set_result_fields(h, 0) == _lib.E_ARG                  # no token bytes
        assert L.dtk_stream_set_result_fields(h, 4 | 2) == _lib.E_ARG             # rune offsets are the host writer's
        assert L.dtk_stream_set_chunking(h, 8, 8) == _lib.E_ARG
        assert L.dtk_stream_run(h, None, _lib.READ_FN(lambda *a: 0), None, 0, _lib.STREAM_SLICE_FN(lambda *a: 0), None,
                                None) == _lib.E_ARG
        L.dtk_stream_free(h)
    L.dtk_stream_free(None)
    assert os.path.exists(os.path.join(MODELS, "tokenizer_de.matok"))
