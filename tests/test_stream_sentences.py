"""A stream's sentences delivered as rows (dtk_stream_set_sentences, dtk_streamsens.hip): the row that is open at a cut
is carried from slice to slice on the device, and every slice brings the rows its calls close.  Every test compares
each slice's rows and both carries with streamsens.sentences_slice_ref of that slice's own arrays and carry-in, so that
a failure names the slice, and the slices' rows joined with the table of the WHOLE stream from the oracle's calls and
rune offsets (streamsens.stream_table)."""
import gzip
import os

import numpy as np
import pytest

import craft
import sentences as sn
import streamcorpus as sc
from streamoffs import offsets_slice_ref
from streampos import CARRY0
from streamsens import SEN_CARRY0, SIX, assert_table, join_sentences, sentences_slice_ref, stream_table
from test_stream import models, whole  # noqa: F401  (fixtures: the device and oracle models, the 200 KB streams)
from test_stream_offsets import oracle_prefix, run_offsets, slice_parts
from test_stream_offsets_host import FIVE, assert_joined
from test_stream_positions_host import empty_text_streams
from test_stream_render import INVALID_MODELS, code_twin, invalid_stream_of

pytestmark = pytest.mark.gpu

S = sc.S
NL = 16
PLAIN, BLOCKED = 0, 1
MODELS_1 = ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_de.datok:pairs", "tokenizer_en.matok"]


def sen_parts(sl):
    return sl.s_tok_end, sl.s_bstart, sl.s_bend, sl.s_rstart, sl.s_rend, sl.s_text_sen_end


def assert_sentences(st, tok, om, raw, nl, offs=None, read_size=None, calls=None, doc=None, carry0=CARRY0, shift=0):
    """Runs `raw` with the sentence rows on `st` -- alone (offs None) or beside offset delivery in the form `offs` --;
    returns the slices.  calls / doc: the oracle's for the whole stream (default: computed here); shift: what the run adds
    to the rune spans of the stream's first text (SP_POSC0)."""
    is_matrix = tok.type() == "MATOK"
    st.set_offsets(offs)
    st.set_sentences(True)
    slices, status = run_offsets(st, tok, raw, nl, read_size)
    sc.check_slices(slices, len(raw))
    carry, sen = carry0, SEN_CARRY0
    for i, sl in enumerate(slices):
        where = "slice %d of %d (base %d, %d tokens, %d entries, carry_in %r / %r), nl %d, offsets %r" % (
            i, len(slices), sl.base, len(sl.tok_bend), len(sl.evl_pos), carry, sl.s_carry_in, nl, offs)
        assert sl.s_tok_end is not None and sl.s_carry_in == sen, (where, sen)
        assert sl.s_tok_end.dtype == np.uint32 and sl.s_bstart.dtype == np.uint64 and sl.s_rstart.dtype == np.int64
        o = offsets_slice_ref(is_matrix, sl, nl, carry)
        ref = sentences_slice_ref(is_matrix, sl, nl, carry, sen)
        assert_table(sen_parts(sl), ref[:6], where)
        assert sl.s_carry_out == ref[6], (where, sl.s_carry_out, ref[6])
        assert sl.s_carry_out[0] == (not o[5][1] and not sl.last), where       # open == !sentB of the writer's carry
        if offs is None:
            assert sl.r_tok_rstart is None and sl.r_sent is None and sl.r_carry_out is None, where
        else:                                                                  # the offsets beside them are as ever
            assert sl.r_carry_in == carry and sl.r_blocked == bool(offs), where
            for name, got, want in zip(FIVE, slice_parts(sl), o):
                assert len(got) == len(want), (where, name, len(got), len(want))
                assert np.array_equal(np.asarray(got, np.int64), np.asarray(want, np.int64)), (where, name)
            assert sl.r_carry_out == o[5], where
        carry, sen = o[5], sl.s_carry_out
    assert sen == SEN_CARRY0
    if calls is None:
        calls = sc.oracle_calls(om, raw)[0]
    if doc is None:
        doc = om.transduce_doc(raw, nl)
    got = join_sentences([(len(sl.tok_bend),) + sen_parts(sl) for sl in slices])
    if status & sc.ST_WINDOW_OVERFLOW:
        # the reference ends at the token that fits no window: the rows that end in front of it
        nt = oracle_prefix(om, raw)[0]
        want = stream_table(calls, doc, n_tok=nt)
        n = int(np.sum(want[0] < nt))
        assert n > 10 and len(got[0]) >= n
        assert_table([g[:n] for g in got], [w[:n] for w in want], (nl, offs), only=("sen_tok_end",))
        return slices
    want = list(stream_table(calls, doc))
    if shift:
        first_text = int(want[5][0]) if len(want[5]) else len(want[0])
        want[3][:first_text] += shift; want[4][:first_text] += shift
    assert_table(got, want, (nl, offs))
    if offs is not None and not shift:
        assert_joined([slice_parts(sl) for sl in slices], doc, (nl, offs))
    return slices


def spans(slices):
    """rows that take tokens on both sides of a cut / carried rows closed without a token of the delivering slice"""
    both = sum(1 for sl in slices if sl.s_carry_in[0] and len(sl.s_tok_end) and sl.s_tok_end[0] > 0)
    none = sum(1 for sl in slices if sl.s_carry_in[0] and len(sl.s_tok_end) and sl.s_tok_end[0] == 0)
    return both, none


# ---- 1. the 200 KB streams
@pytest.mark.parametrize("name", MODELS_1)
def test_rows_equal_the_streams_table(models, whole, name):
    import datok_amd
    tok, om = models(name)
    raw, calls, _ = whole("en" if "_en" in name else "de", name.partition(":")[0], om)
    docs = {nl: om.transduce_doc(raw, nl) for nl in (0, NL)}
    assert all(d.status == 0 for d in docs.values())
    for depth in (3, 2):
        with datok_amd.Stream(S, depth=depth) as st:
            for nl in (0, NL):
                for offs in (None, BLOCKED):
                    slices = assert_sentences(st, tok, om, raw, nl, offs, read_size=5000, calls=calls, doc=docs[nl])
                    assert len(slices) >= 12 and sum(len(sl.s_text_sen_end) for sl in slices) >= 10
                    assert spans(slices)[0] >= 1


# ---- 2. every alignment of a cut
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
@pytest.mark.parametrize("construct", list(sc.CONSTRUCTS))
def test_cut_alignment(models, name, construct):
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for shift in (0, 1, 2, 3, 39):
            raw = sc.construct_stream(construct, shift)
            calls, status = sc.oracle_calls(om, raw)
            assert construct == "token5000" or status == 0
            for nl, offs in ((0, None), (NL, BLOCKED)):
                slices = assert_sentences(st, tok, om, raw, nl, offs, calls=calls)
            if construct == "token5000":
                assert slices[-1].status & sc.ST_WINDOW_OVERFLOW


# ---- 3. a text that spans five slices
def test_a_text_of_five_slices(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = sc.running_text(5 * S, seed=21).replace(b"\x04", b" ")
    assert om.transduce_doc(raw, 0).status == 0
    with datok_amd.Stream(S) as st:
        for offs in (None, PLAIN):
            slices = assert_sentences(st, tok, om, raw, 0, offs)
            assert len(slices) == 5
            assert all(len(sl.s_text_sen_end) == 0 for sl in slices[:-1]) and len(slices[-1].s_text_sen_end) == 1
            assert slices[-1].s_text_sen_end[0] == len(slices[-1].s_tok_end)
            if offs is not None:
                assert all(sl.s_carry_out[0] == (not sl.r_carry_out[1]) for sl in slices[:-1])
            assert slices[-1].s_carry_out == SEN_CARRY0


# ---- 4. counts at the kernels' edges
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 4096])
def test_token_counts_at_the_tile_and_block_edges(models, n):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b"a " * n
    doc = om.transduce_doc(raw, 0)
    assert doc.status == (0 if n else sc.ST_EMPTY_TEXT) and len(doc.tok_rstart) == n
    with datok_amd.Stream(S) as st:
        for offs in (None, BLOCKED):
            slices = assert_sentences(st, tok, om, raw, 0, offs, doc=doc)
            assert len(slices) == 1 and slices[0].s_tok_end.tolist() == ([n] if n else [])    # one row of n tokens, or none
            assert slices[0].s_text_sen_end.tolist() == [1 if n else 0]


@pytest.mark.parametrize("raw,n_tok,firsts", [
    (b"Ja. " * 128 + b"a " * 3, 259, (254, 256)),                 # a row ends with the tile's last token, the next tile begins one
    (b"Es geht. " + b"Ja. " * 127 + b"a ", 258, (255, 257)),      # a row begins with the tile's last token
    (b"Ja. " * 600, 1200, (1022, 1024, 1026)),                    # ... and the same at the scanning block's 1024
])
def test_a_sentence_first_token_on_either_side_of_a_tile_edge(models, raw, n_tok, firsts):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    calls = sc.oracle_calls(om, raw)[0]
    f, n = sn.from_calls(calls)
    assert n == n_tok and set(firsts) <= set(f) and not any(x + 1 in f for x in firsts)
    with datok_amd.Stream(S) as st:
        for offs in (None, BLOCKED):
            slices = assert_sentences(st, tok, om, raw, 0, offs, calls=calls)
            assert len(slices) == 1 and slices[0].s_tok_end.tolist() == f[1:] + [n]


# ---- 5. dense sentences, no token at all
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_dense_sentences_blanks_and_the_empty_stream(models, name):
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for raw in (b"a b. " * 8000, b"Es geht so. " * 3400):
            assert om.transduce_doc(raw, 0).status == 0
            for nl, offs in ((0, None), (NL, BLOCKED)):
                slices = assert_sentences(st, tok, om, raw, nl, offs)
            assert len(slices) >= 2 and len(slices[0].tok_bend) > 4000
        assert len(slices[0].evl_pos) > 1000 and len(slices[0].s_tok_end) > 1000
        for raw in (b" " * 1000, b""):                           # no token: no row, one text row
            for offs in (None, BLOCKED):
                slices = assert_sentences(st, tok, om, raw, 0, offs)
                assert len(slices) == 1 and len(slices[0].s_tok_end) == 0 and slices[0].s_text_sen_end.tolist() == [0]


# ---- 6. bytes that do not decode
@pytest.mark.parametrize("name", INVALID_MODELS)
def test_invalid_utf8_counts_as_one_rune_a_byte(models, name):
    import datok_amd
    tok, om = models(name)
    raw = invalid_stream_of(name)
    assert om.transduce_doc(raw, 0).status == 0
    mine = {}
    with datok_amd.Stream(S) as st:
        for nl, offs in ((0, None), (NL, BLOCKED)):
            slices = mine[offs] = assert_sentences(st, tok, om, raw, nl, offs)
        assert len(slices) == 5 if name != "de64.matok" else len(slices) >= 4
        assert all(sl.out is None for sl in slices)       # (no bytes are rendered here: the rows' rune spans read the stream)
    twin = code_twin(models, name)
    if twin is not None:          # the same automaton and the same stream: any difference is the stream format's
        with datok_amd.Stream(S) as st:
            for nl, offs in ((0, None), (NL, BLOCKED)):
                for a, b in zip(assert_sentences(st, twin, om, raw, nl, offs), mine[offs]):
                    assert all(np.array_equal(x, y) for x, y in zip(sen_parts(a), sen_parts(b)))
                    assert (a.s_carry_in, a.s_carry_out) == (b.s_carry_in, b.s_carry_out)


# ---- 7. later work on a slice
@pytest.mark.parametrize("chunk,warm", [(16, 0), (0, 8)])
def test_repair_rounds_and_one_lane_per_slice(models, whole, chunk, warm):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw, calls, _ = whole("de", "tokenizer_de.matok", om)
    with datok_amd.Stream(S) as st:
        st.set_chunking(chunk, warm)
        assert_sentences(st, tok, om, raw, NL, None, calls=calls)


# ---- 8. a slice computed twice, rows that come late
def test_a_slice_computed_twice_leaves_the_same_rows_and_carries(models, whole):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw, calls, _ = whole("de", "tokenizer_de.matok", om)
    doc = om.transduce_doc(raw, 0)
    with datok_amd.Stream(S) as st:
        for offs in (None, BLOCKED):
            plain = assert_sentences(st, tok, om, raw, 0, offs, calls=calls, doc=doc)
            assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"1") == 0
            try:
                slices = assert_sentences(st, tok, om, raw, 0, offs, calls=calls, doc=doc)
            finally:
                assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", os.environ.get("DATOK_EVL_CAP", "-1").encode()) == 0
            assert sum(len(sl.evl_pos) > 1 for sl in slices) >= 10 and sum(len(sl.s_tok_end) > 1 for sl in slices) >= 10
            assert [(sl.s_carry_in, sl.s_carry_out) for sl in slices] == [(sl.s_carry_in, sl.s_carry_out) for sl in plain]
            for a, b in zip(slices, plain):
                assert all(np.array_equal(x, y) for x, y in zip(sen_parts(a), sen_parts(b)))


def many_texts(total=40 * 1024, every=2048):
    """Running text with a text end (U+0004) behind a sentence end about every `every` bytes."""
    raw = sc.running_text(total, seed=5)
    parts, at = [], 0
    while (k := raw.find(b". ", at + every)) >= 0:
        parts.append(raw[at:k + 1] + b"\x04")
        at = k + 1
    return b"".join(parts) + raw[at:]


def test_every_array_of_a_slice_comes_late(models):
    """Several texts in a slice: where the first copies are sized for one element (EVL_CAP=1), the text rows, the sent ints
    and the sentence rows of both tables all have elements that only the delivery brings."""
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = many_texts()
    calls, doc = sc.oracle_calls(om, raw)[0], om.transduce_doc(raw, 0)
    assert doc.status == 0
    with datok_amd.Stream(16384) as st:
        plain = assert_sentences(st, tok, om, raw, 0, BLOCKED, calls=calls, doc=doc)
        assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"1") == 0
        try:
            late = assert_sentences(st, tok, om, raw, 0, BLOCKED, calls=calls, doc=doc)
        finally:
            assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", os.environ.get("DATOK_EVL_CAP", "-1").encode()) == 0
    assert any(min(len(sl.r_text_tok_end), len(sl.s_text_sen_end), len(sl.r_sent), len(sl.s_tok_end)) >= 3 for sl in plain)
    assert len(late) == len(plain) >= 2
    for a, b in zip(late, plain):
        assert (a.s_carry_in, a.s_carry_out, a.r_carry_in, a.r_carry_out) == (b.s_carry_in, b.s_carry_out, b.r_carry_in, b.r_carry_out)
        assert all(np.array_equal(x, y) for x, y in zip(sen_parts(a) + slice_parts(a), sen_parts(b) + slice_parts(b)))
        assert a.r_blocked == b.r_blocked and np.array_equal(a.r_rblk, b.r_rblk) and np.array_equal(a.r_rblk_head, b.r_rblk_head)


# ---- 9. beyond 32 bits
def test_rune_spans_beyond_32_bits(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    base = 9999999950
    L = datok_amd.lib()
    with datok_amd.Stream(S) as st:
        for raw in (b"Ja. " * 100, b"Ja. a b c\x04\n" * 50):        # one text; fifty, of which only the first feels the carried posC
            for offs in (None, BLOCKED):
                assert L.dtk_debug_configure(b"SP_POSC0", str(base).encode()) == 0
                try:
                    slices = assert_sentences(st, tok, om, raw, 0, offs, carry0=(base, True, True, False, False), shift=base)
                finally:
                    assert L.dtk_debug_configure(b"SP_POSC0", b"0") == 0
                assert len(slices) == 1 and slices[0].s_rstart[0] > 2 ** 32 and slices[0].s_rend[1] > 2 ** 32
        assert slices[0].s_rstart[2] < 100 and slices[0].s_bstart[2] < 100
        assert_sentences(st, tok, om, raw, 0, None)                 # (the key is read at a run's start: off again)


# ---- 10. empty texts; the literal newline rule a second time
def test_empty_texts_follow_the_oracle(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    none = 0
    with datok_amd.Stream(S) as st:
        for k, (raw, empty) in enumerate(empty_text_streams()):
            doc = om.transduce_doc(raw, 0)
            assert bool(doc.status & sc.ST_EMPTY_TEXT) == empty
            slices = assert_sentences(st, tok, om, raw, 0, BLOCKED if k % 2 else None, doc=doc)
            none += spans(slices)[1]
    assert none >= 1                                                # a carried row closed with no token of the delivering slice


def test_a_token_that_ends_at_zero_under_the_newline_rule_is_refused(tmp_path):
    """test_stream_offsets.py's crafted tokenizer in which a newline begins a word: DTK_E_IRREGULAR where offset delivery
    gives it, and a regular table without the rule."""
    import datok_amd
    from datok_amd import _lib
    from oracle import oracle as O
    arcs = craft._automaton(False)
    for state in (1, 3):
        arcs[state][craft.NL] = (2, False)
    img = craft.matok_from(arcs)
    path = tmp_path / "newline.matok"
    path.write_bytes(img)
    tok = datok_amd.load_tokenizer_file(str(path))
    om = O.Model(raw=gzip.decompress(img))
    raw = b"ab a. \x04\n ab. b \x04\n a" * 8
    doc = om.transduce_doc(raw, NL)
    assert doc.status == 0 and doc.tok_rstart[3] == -1 and doc.tok_rend[3] == 0
    with datok_amd.Stream(S) as st:
        for offs in (None, BLOCKED):
            st.set_offsets(offs)
            st.set_sentences(True)
            with pytest.raises(_lib.DatokGpuError) as e:
                st.run(tok, raw, flags=NL)
            assert e.value.code == _lib.E_IRREGULAR
            assert_sentences(st, tok, om, raw, 0, offs)


# ---- 11. reuse
def test_one_stream_object_through_modes(models, whole):
    import datok_amd
    from datok_amd import _lib
    from test_stream_render import assert_rendered
    tok, om = models("tokenizer_de.matok")
    raw, calls, _ = whole("de", "tokenizer_de.matok", om)
    short = sc.running_text(30000, seed=2)
    with datok_amd.Stream(S) as st:
        st.set_render(3)                                          # the surfaces as text and the sentences as rows
        slices = assert_sentences(st, tok, om, raw, 0, None, calls=calls)
        assert all(sl.out is not None and sl.written is None and sl.r_tok_rstart is None for sl in slices)
        assert b"".join(sl.out for sl in slices) == om.transduce(raw, 3)[0]
        with pytest.raises(_lib.DatokGpuError) as e:              # exclusive with position rendering
            st.set_position_render(15)
        assert e.value.code == _lib.E_ARG
        slices = assert_sentences(st, tok, om, short, NL, None)   # (a refused call changes nothing; a shorter stream starts fresh)
        assert all(sl.out is not None and sl.carry_out is None for sl in slices)
        st.set_sentences(False)
        for sl in assert_rendered(st, tok, om, short, 3):
            assert all(getattr(sl, k) is None for k in sl.__slots__ if k.startswith("s_")) and sl.r_sent is None
        st.set_position_render(15)
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_sentences(True)
        assert e.value.code == _lib.E_ARG
        st.set_position_render(None)
        assert_sentences(st, tok, om, short, 0, PLAIN)
        assert st.transduce(tok, raw, 15) == om.transduce(raw, 15)
        got = []
        st.run(tok, raw, on_slice=got.append)                     # dtk_stream_transduce leaves the rows off
        assert got and all(sl.s_tok_end is None and sl.r_tok_rstart is None and sl.out is None for sl in got)
