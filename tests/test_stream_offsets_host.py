"""Offset delivery's specification without a GPU: streamoffs.offsets_slice_ref -- the integers a writer with TOKEN_POS |
SENTENCE_POS collects during one slice's calls, from the state carried in -- on synthetic slice views cut from the
oracle's calls.  The slices' arrays joined are the oracle's arrays for the whole stream (oracle.Model.transduce_doc),
every slice's carry_out is the state of the C++ mirror's writer behind it, and the blocked form round-trips."""
import io

import numpy as np
import pytest

import streamcorpus as sc
from streamoffs import (HEAD64, SPAN, join_slices, offsets_slice_ref, pack_blocked64_ref, unpack_blocked64_ref)
from streampos import CARRY0, mirror_token_writer
from test_stream_positions_host import empty_text_streams

MODELS = ["tokenizer_de.matok", "tokenizer_de.datok"]
NL = 16
FIVE = ("tok_rstart", "tok_rend", "sent", "text_tok_end", "text_sent_end")


def assert_joined(parts, doc, what=()):
    """The slices' arrays, joined, against a DocResult of the whole stream."""
    got = join_slices(parts)
    for name, g in zip(FIVE, got):
        want = np.asarray(getattr(doc, name), np.int64)
        assert len(g) == len(want), (what, name, len(g), len(want))
        bad = np.flatnonzero(g != want)
        assert len(bad) == 0, (what, name, int(bad[0]), g[bad[:3]], want[bad[:3]])


def _check(om, raw, empty_text=False):
    from datok_amd import host
    is_matrix = om.type() == "MATOK"
    calls, st = sc.oracle_calls(om, raw)
    assert st == (sc.ST_EMPTY_TEXT if empty_text else 0) or raw.count(b"a" * 5000)
    slices = sc.synthetic_slices(is_matrix, raw, calls, sc.S)
    assert len(slices) >= 2
    for nl in (0, NL):
        carry, parts = CARRY0, []
        tw, state = mirror_token_writer(io.BytesIO(), 12 | nl)
        for i, sl in enumerate(slices):
            r = offsets_slice_ref(is_matrix, sl, nl, carry)
            parts.append(r)
            host.replay_slice(is_matrix, sl, tw)
            carry = r[5]
            assert carry == (state["posC"], state["sentB"], state["init"], bool(state["pos"]), bool(state["sent"])), (nl, i)
            assert len(r[0]) == len(r[1]) == len(sl.tok_bend) and len(r[3]) == len(r[4])
        doc = om.transduce_doc(raw, nl)
        assert bool(doc.status & sc.ST_EMPTY_TEXT) == empty_text
        assert_joined(parts, doc, nl)


@pytest.mark.parametrize("model", MODELS)
def test_reference_joins_to_the_oracles_arrays_on_the_200k_stream(oracle_models, model):
    om = oracle_models(model)
    raw = sc.running_text(200 * 1024, seed=5)
    assert raw.count(b"\x04") >= 10
    _check(om, raw)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("construct", list(sc.CONSTRUCTS))
def test_reference_joins_at_every_cut_alignment(oracle_models, model, construct):
    om = oracle_models(model)
    for shift in (0, 1, 2, 3, 39):
        _check(om, sc.construct_stream(construct, shift))


@pytest.mark.parametrize("model", MODELS)
def test_reference_skips_the_push_of_an_empty_text(oracle_models, model):
    om = oracle_models(model)
    for raw, empty in empty_text_streams():
        _check(om, raw, empty_text=empty)


def test_a_text_end_right_behind_the_cut():
    """One slice by hand (test_stream_positions_host.py's): the TextEnd of a text that began earlier fires before any
    token of this slice; the SentenceEnd in front of it pushes the carried posC."""
    from datok_amd import host
    text = b"x.\x04\nab c"
    sl = host.SliceView(base=16384, first=2, cut=len(text), last=1, status=0, text=text,
                        tok_bstart=np.array([4, 7], np.uint32), tok_bend=np.array([6, 8], np.uint32),
                        evl_pos=np.array([3], np.uint32), evl_kind=np.array([host.EVL_SEOT | host.EVL_TEOT], np.uint8),
                        tail=len(text) << 2 | 3)
    carry = (7, False, False, True, True)
    rs, re, sent, tte, tse, out = offsets_slice_ref(True, sl, 0, carry)
    assert (rs.tolist(), re.tolist(), sent.tolist()) == ([1, 4], [3, 5], [7, 1, 5])
    assert (tte.tolist(), tse.tolist(), out) == ([0, 2], [1, 3], (0, True, False, False, False))
    rs, re, sent, _, _, _ = offsets_slice_ref(True, sl, NL, carry)      # the newline rule at the slice's first token
    assert (rs.tolist(), re.tolist(), sent.tolist()) == ([0, 3], [2, 4], [7, 0, 4])
    sl.last, sl.tail = 0, 0                                             # the text stays open without the tail
    r = offsets_slice_ref(True, sl, 0, carry)
    assert r[3].tolist() == [0] and r[5] == (5, False, False, True, True)
    # an empty text: the carried text has no token, so the SentenceEnd pushes nothing
    r = offsets_slice_ref(True, sl, 0, (0, True, False, False, False))
    assert r[2].tolist() == [1] and r[4].tolist() == [0]


def test_blocked_reference_round_trips_and_refuses_a_wide_block():
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, 200):
        for base in (0, 9999999950, -1):
            # texts of a few tokens each: offsets grow inside a text and start again at its first token
            start, end, pos = [], [], base
            for i in range(n):
                if i and rng.integers(0, 9) == 0:
                    pos = int(rng.integers(-1, 3))
                pos += int(rng.integers(0, 5))
                start.append(pos)
                pos += int(rng.integers(0, 30))
                end.append(pos)
            words, heads = pack_blocked64_ref(start, end)
            assert words.dtype == np.uint32 and heads.dtype == HEAD64 and HEAD64.itemsize == 24
            assert len(words) == n and len(heads) == (n + 63) // 64
            s, e = unpack_blocked64_ref(words, heads)
            assert s.tolist() == start and e.tolist() == end
            from datok_amd import host
            s, e = host.unpack_blocked64(words, heads)
            assert s.dtype == np.int64 and s.tolist() == start and e.tolist() == end
    # one break per block: the first token that starts before its predecessor's end
    words, heads = pack_blocked64_ref([10, 12, 0, 3, 1], [11, 14, 2, 4, 2])
    assert heads[0].tolist() == (10, 0, 2, 0)
    assert unpack_blocked64_ref(words, heads)[0].tolist() == [10, 12, 0, 3, 1]
    # a segment that spans more than 16 bits does not fit: the limit itself does
    pack_blocked64_ref([0, SPAN - 1], [1, SPAN])
    with pytest.raises(ValueError):
        pack_blocked64_ref([0, SPAN], [1, SPAN + 1])
    with pytest.raises(ValueError):
        pack_blocked64_ref([2 ** 40, 5, 4, 2 ** 40], [2 ** 40 + 1, 6, 5, 2 ** 40 + 1])   # the second segment holds both
    with pytest.raises(ValueError):
        pack_blocked64_ref([0, 17], [1, 18], span=16)


def test_set_offsets_checks_its_arguments():
    import ctypes as C
    import datok_amd
    from datok_amd import _lib
    L = datok_amd.lib()
    for name in ("dtk_stream_set_offsets", "dtk_stream_offsets", "dtk_blk64_start", "dtk_blk64_end"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.dtk_stream_set_offsets(None, 1, _lib.SO_PLAIN) == _lib.E_ARG
    assert L.dtk_stream_offsets(None, None) == _lib.E_ARG
    assert C.sizeof(_lib.StreamOffs) == 3 * 8 + 7 * 8 + 2 * 24
    # the exported decoders on a block by the reference packer
    start, end = [9999999950, 9999999952, 0, 2], [9999999951, 9999999953, 1, 3]
    words, heads = pack_blocked64_ref(start, end)
    for i in range(4):
        assert L.dtk_blk64_start(words.ctypes.data, heads.ctypes.data, i) == start[i]
        assert L.dtk_blk64_end(words.ctypes.data, heads.ctypes.data, i) == end[i]
    h = C.c_void_p()
    if L.dtk_device_count() > 0:
        assert L.dtk_stream_create(16384, 3, C.byref(h)) == _lib.OK
        assert L.dtk_stream_set_offsets(h, 1, 2) == _lib.E_ARG
        assert L.dtk_stream_set_offsets(h, 1, _lib.SO_BLOCKED) == _lib.OK
        assert L.dtk_stream_set_position_render(h, 1, 12) == _lib.E_ARG
        so = _lib.StreamOffs()
        assert L.dtk_stream_offsets(h, C.byref(so)) == _lib.E_STATE      # (outside slice_fn)
        assert L.dtk_stream_set_offsets(h, 0, 0) == _lib.OK
        assert L.dtk_stream_set_position_render(h, 1, 12) == _lib.OK
        assert L.dtk_stream_set_offsets(h, 1, _lib.SO_PLAIN) == _lib.E_ARG
        L.dtk_stream_free(h)
