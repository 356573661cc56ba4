"""A stream's rune offsets and sentence list delivered as arrays (dtk_stream_set_offsets, dtk_streamoffs.hip): the
writer's state is carried from slice to slice on the device, and every slice brings what a writer with TOKEN_POS |
SENTENCE_POS collects during its calls.  Every test compares each slice's arrays and carry_out with
streamoffs.offsets_slice_ref of that slice's own arrays and carry_in, so that a failure names the slice, and the slices'
arrays joined with the oracle's arrays for the WHOLE stream (oracle.Model.transduce_doc)."""
import gzip
import io
import os

import numpy as np
import pytest

import craft
import streamcorpus as sc
from streamoffs import join_slices, offsets_slice_ref, pack_blocked64_ref
from streampos import CARRY0
from test_stream import models, whole  # noqa: F401  (fixtures: the device and oracle models, the 200 KB streams)
from test_stream_offsets_host import FIVE, assert_joined
from test_stream_positions_host import empty_text_streams
from test_stream_render import INVALID_MODELS, code_twin, invalid_stream_of

pytestmark = pytest.mark.gpu

S = sc.S
NL = 16
PLAIN, BLOCKED = 0, 1
MODELS_1 = ["tokenizer_de.matok", "tokenizer_de.datok", "tokenizer_de.datok:pairs", "tokenizer_en.matok"]


def run_offsets(st, tok, raw, nl, read_size=None):
    r = io.BytesIO(raw)
    if read_size:
        class Short:
            def read(self, n):
                return r.read(min(n, read_size))
        reader = Short()
    else:
        reader = r
    slices = []
    status = st.run(tok, reader, flags=nl, on_slice=slices.append)
    return slices, status


def slice_parts(sl):
    return sl.r_tok_rstart, sl.r_tok_rend, sl.r_sent, sl.r_text_tok_end, sl.r_text_sent_end


def oracle_prefix(om, raw):
    """(tokens, sent ints, texts) a writer has collected when the reference's window overflows: the oracle's calls in
    front of the token that fits no window (test_stream.py, assert_stream)."""
    calls = sc.oracle_calls(om, raw)[0]
    n = next(i for i, c in enumerate(calls) if c[0] == 0 and c[4] - c[2] > 4104)
    assert n > 100
    nt = ns = nx = 0
    sentB, has_tok = True, False
    for c in calls[:n]:
        if c[0] == 0:
            nt += 1
            ns += sentB
            sentB, has_tok = False, True
        elif c[0] == 1:
            ns += has_tok
            sentB = True
        else:
            nx += 1
            sentB, has_tok = True, False
    return nt, ns, nx


class _Doc:
    pass


def _cut(doc, nt, ns, nx):
    d = _Doc()
    d.tok_rstart, d.tok_rend, d.sent = doc.tok_rstart[:nt], doc.tok_rend[:nt], doc.sent[:ns]
    d.text_tok_end, d.text_sent_end = doc.text_tok_end[:nx], doc.text_sent_end[:nx]
    return d


def assert_offsets(st, tok, om, raw, nl, form, read_size=None, doc=None, carry0=CARRY0, blocked=None):
    """Runs `raw` with offset delivery in `form` on `st`; returns the slices.  doc: what the joined arrays must equal
    (default: the oracle's for the whole stream); blocked: the form that must come (default: the one asked for)."""
    is_matrix = tok.type() == "MATOK"
    st.set_offsets(form)
    slices, status = run_offsets(st, tok, raw, nl, read_size)
    sc.check_slices(slices, len(raw))
    carry = carry0
    for i, sl in enumerate(slices):
        where = "slice %d of %d (base %d, %d tokens, %d entries, carry_in %r), nl %d, form %d" % (
            i, len(slices), sl.base, len(sl.tok_bend), len(sl.evl_pos), sl.r_carry_in, nl, form)
        assert sl.r_tok_rstart is not None and sl.r_carry_in == carry, (where, carry)
        assert sl.r_blocked == (bool(form) if blocked is None else blocked), where
        assert sl.r_tok_rstart.dtype == np.int64 and sl.r_sent.dtype == np.int64
        ref = offsets_slice_ref(is_matrix, sl, nl, sl.r_carry_in)
        for name, got, want in zip(FIVE, slice_parts(sl), ref):
            assert len(got) == len(want), (where, name, len(got), len(want))
            bad = np.flatnonzero(np.asarray(got, np.int64) != np.asarray(want, np.int64))
            assert len(bad) == 0, (where, name, int(bad[0]), got[bad[:3]], want[bad[:3]])
        assert sl.r_carry_out == ref[5], (where, sl.r_carry_out, ref[5])
        carry = sl.r_carry_out
    if doc is None:
        doc = om.transduce_doc(raw, nl)
    parts = [slice_parts(sl) for sl in slices]
    if status & sc.ST_WINDOW_OVERFLOW:
        nt, ns, nx = oracle_prefix(om, raw)
        j = join_slices(parts)
        assert len(j[0]) >= nt and len(j[2]) >= ns and len(j[3]) >= nx
        parts = [(j[0][:nt], j[1][:nt], j[2][:ns], j[3][:nx], j[4][:nx])]
        doc = _cut(doc, nt, ns, nx)
    assert_joined(parts, doc, (nl, form))
    return slices


# ---- 1. the 200 KB streams
@pytest.mark.parametrize("name", MODELS_1)
def test_offsets_equal_the_oracles_arrays(models, whole, name):
    import datok_amd
    tok, om = models(name)
    raw = whole("en" if "_en" in name else "de", name.partition(":")[0], om)[0]
    docs = {nl: om.transduce_doc(raw, nl) for nl in (0, NL)}
    assert all(d.status == 0 for d in docs.values())
    for depth in (3, 2):
        with datok_amd.Stream(S, depth=depth) as st:
            for nl in (0, NL):
                for form in (PLAIN, BLOCKED):
                    slices = assert_offsets(st, tok, om, raw, nl, form, read_size=5000, doc=docs[nl])
                    assert len(slices) >= 12 and sum(len(sl.r_text_tok_end) for sl in slices) >= 10


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
            for nl, form in ((0, PLAIN), (NL, BLOCKED)):
                slices = assert_offsets(st, tok, om, raw, nl, form)
            if construct == "token5000":
                assert slices[-1].status & sc.ST_WINDOW_OVERFLOW
            elif construct == "token4000":
                assert any(int(e) - int(b) == 1000 for sl in slices for b, e in zip(sl.r_tok_rstart, sl.r_tok_rend))


# ---- 3. a text that spans five slices
def test_a_text_of_five_slices(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = sc.running_text(5 * S, seed=21).replace(b"\x04", b" ")
    assert om.transduce_doc(raw, 0).status == 0
    with datok_amd.Stream(S) as st:
        for form in (PLAIN, BLOCKED):
            slices = assert_offsets(st, tok, om, raw, 0, form)
            assert len(slices) == 5
            assert all(len(sl.r_text_tok_end) == 0 for sl in slices[:-1]) and len(slices[-1].r_text_tok_end) == 1
            posc = [sl.r_carry_out[0] for sl in slices[:-1]]
            assert posc == sorted(posc) and posc[0] > S * 0.8 and posc[-1] > 4 * S * 0.8
            assert all(sl.r_carry_out[3] for sl in slices[:-1]) and slices[-1].r_carry_out == (0, True, False, False, False)


# ---- 4. beyond 32 bits
def _with_posc0(base, fn):
    import datok_amd
    L = datok_amd.lib()
    assert L.dtk_debug_configure(b"SP_POSC0", str(base).encode()) == 0
    try:
        return fn()
    finally:
        assert L.dtk_debug_configure(b"SP_POSC0", b"0") == 0


def test_offsets_beyond_32_bits(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    base = 9999999950
    carry0 = (base, True, True, False, False)
    with datok_amd.Stream(S) as st:
        # one text: every integer lies `base` further on
        raw = b"a " * 200
        doc = om.transduce_doc(raw, 0)
        assert doc.status == 0 and len(doc.tok_rstart) == 200 and len(doc.text_tok_end) == 1
        want = _cut(doc, 200, len(doc.sent), 1)
        want.tok_rstart, want.tok_rend, want.sent = (np.asarray(x, np.int64) + base for x in (doc.tok_rstart, doc.tok_rend, doc.sent))
        assert want.tok_rend[24] == 9999999999 and want.tok_rstart[25] == 10000000000 and want.tok_rstart[0] > 2 ** 32
        for form in (PLAIN, BLOCKED):
            slices = _with_posc0(base, lambda: assert_offsets(st, tok, om, raw, 0, form, doc=want, carry0=carry0))
            assert len(slices) == 1
        heads = slices[0].r_rblk_head
        assert len(heads) == 4 and all(int(h["base0"]) > 2 ** 32 and int(h["brk"]) == 64 for h in heads)
        assert_offsets(st, tok, om, raw, 0, BLOCKED)                # (the key is read at a run's start: off again)
        # fifty texts: only the first one feels the carried posC; the newline rule's -1 shows in base1
        raw = b"a b c\x04\n" * 50
        for nl in (NL, 0):
            doc = om.transduce_doc(raw, nl)
            assert doc.status == 0 and doc.text_tok_end[:2].tolist() == [3, 6]
            want = _cut(doc, len(doc.tok_rstart), len(doc.sent), len(doc.text_tok_end))
            want.tok_rstart, want.tok_rend, want.sent = (np.asarray(x, np.int64).copy() for x in (doc.tok_rstart, doc.tok_rend, doc.sent))
            want.tok_rstart[:3] += base; want.tok_rend[:3] += base; want.sent[:int(doc.text_sent_end[0])] += base
            slices = _with_posc0(base, lambda: assert_offsets(st, tok, om, raw, nl, BLOCKED, doc=want, carry0=carry0))
            h = slices[0].r_rblk_head[0]
            assert int(h["brk"]) == 3 and int(h["base0"]) == base and int(h["base1"]) == (0 if nl else 1)
            w, hh = pack_blocked64_ref(slices[0].r_tok_rstart, slices[0].r_tok_rend)
            assert np.array_equal(w, slices[0].r_rblk) and hh.tobytes() == slices[0].r_rblk_head.tobytes()
            s_, e_ = slices[0].r_tok_rstart, slices[0].r_tok_rend
            L = datok_amd.lib()
            for i in (0, 2, 3, 63, 64, len(s_) - 1):      # the exported decoders on what the device packed
                assert L.dtk_blk64_start(slices[0].r_rblk.ctypes.data, slices[0].r_rblk_head.ctypes.data, i) == s_[i]
                assert L.dtk_blk64_end(slices[0].r_rblk.ctypes.data, slices[0].r_rblk_head.ctypes.data, i) == e_[i]


# ---- 5. counts at the kernels' edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096])
def test_token_counts_at_the_tile_and_block_edges(models, n):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = b"a " * n
    doc = om.transduce_doc(raw, 0)
    assert doc.status == (0 if n else sc.ST_EMPTY_TEXT) and len(doc.tok_rstart) == n
    with datok_amd.Stream(S) as st:
        for form in (PLAIN, BLOCKED):
            slices = assert_offsets(st, tok, om, raw, 0, form, doc=doc)
            assert len(slices) == 1 and len(slices[0].r_tok_rstart) == n
            if form == BLOCKED:
                assert len(slices[0].r_rblk) == n and len(slices[0].r_rblk_head) == (n + 63) // 64


# ---- 6. dense sentences, no token at all
@pytest.mark.parametrize("name", ["tokenizer_de.matok", "tokenizer_de.datok"])
def test_dense_sentences_blanks_and_the_empty_stream(models, name):
    import datok_amd
    tok, om = models(name)
    with datok_amd.Stream(S) as st:
        for raw in (b"a b. " * 8000, b"Es geht so. " * 3400):   # the second: a sentence integer at almost every other token
            assert om.transduce_doc(raw, 0).status == 0
            for nl, form in ((0, PLAIN), (NL, BLOCKED)):
                slices = assert_offsets(st, tok, om, raw, nl, form)
            assert len(slices) >= 2 and len(slices[0].r_tok_rstart) > 4000
        assert len(slices[0].evl_pos) > 1000 and len(slices[0].r_sent) > 2000
        for raw in (b" " * 1000, b""):                           # no token: no integer, one text row
            for form in (PLAIN, BLOCKED):
                slices = assert_offsets(st, tok, om, raw, 0, form)
                assert len(slices) == 1 and len(slices[0].r_tok_rstart) == 0 and len(slices[0].r_sent) == 0
                assert slices[0].r_text_tok_end.tolist() == [0] and slices[0].r_text_sent_end.tolist() == [0]


# ---- 7. bytes that do not decode
@pytest.mark.parametrize("name", INVALID_MODELS)
def test_invalid_utf8_counts_as_one_rune_a_byte(models, name):
    import datok_amd
    tok, om = models(name)
    raw = invalid_stream_of(name)
    assert om.transduce_doc(raw, 0).status == 0
    mine = {}
    with datok_amd.Stream(S) as st:
        for nl, form in ((0, PLAIN), (NL, BLOCKED)):
            slices = mine[form] = assert_offsets(st, tok, om, raw, nl, form)
        assert len(slices) == 5 if name != "de64.matok" else len(slices) >= 4
        # (no bytes are rendered here: the arrays count an invalid byte as one rune, dtk_sym_is_start's two branches)
        assert all(sl.out is None for sl in slices)
    twin = code_twin(models, name)
    if twin is not None:          # the same automaton and the same stream: any difference is the stream format's
        with datok_amd.Stream(S) as st:
            for nl, form in ((0, PLAIN), (NL, BLOCKED)):
                for a, b in zip(assert_offsets(st, twin, om, raw, nl, form), mine[form]):
                    assert all(np.array_equal(x, y) for x, y in zip(slice_parts(a), slice_parts(b)))
                    assert a.r_carry_out == b.r_carry_out


# ---- 8. later work on a slice
@pytest.mark.parametrize("chunk,warm", [(16, 0), (0, 8)])
def test_repair_rounds_and_one_lane_per_slice(models, whole, chunk, warm):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    with datok_amd.Stream(S) as st:
        st.set_chunking(chunk, warm)
        assert_offsets(st, tok, om, raw, NL, BLOCKED)


# ---- 9. a slice computed twice
def test_a_slice_computed_twice_leaves_the_same_arrays_and_carry(models, whole):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    with datok_amd.Stream(S) as st:
        for form in (PLAIN, BLOCKED):
            plain = assert_offsets(st, tok, om, raw, 0, form)
            assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", b"1") == 0
            try:
                slices = assert_offsets(st, tok, om, raw, 0, form)
            finally:
                assert datok_amd.lib().dtk_debug_configure(b"EVL_CAP", os.environ.get("DATOK_EVL_CAP", "-1").encode()) == 0
            assert sum(len(sl.evl_pos) > 1 for sl in slices) >= 10
            assert [sl.r_carry_out for sl in slices] == [sl.r_carry_out for sl in plain]
            for a, b in zip(slices, plain):
                assert all(np.array_equal(x, y) for x, y in zip(slice_parts(a), slice_parts(b)))


# ---- 10. empty texts
def test_empty_texts_skip_the_push_as_the_oracle_does(models):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    with datok_amd.Stream(S) as st:
        for k, (raw, empty) in enumerate(empty_text_streams()):
            doc = om.transduce_doc(raw, 0)
            assert bool(doc.status & sc.ST_EMPTY_TEXT) == empty
            slices = assert_offsets(st, tok, om, raw, 0, BLOCKED if k % 2 else PLAIN, doc=doc)
            status = 0
            for sl in slices:
                status |= sl.status
            assert bool(status & sc.ST_EMPTY_TEXT) == empty


# ---- 11. a block that does not fit
def test_a_wide_block_brings_the_plain_arrays(models, whole):
    import datok_amd
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    L = datok_amd.lib()
    with datok_amd.Stream(S) as st:
        fit = assert_offsets(st, tok, om, raw, 0, BLOCKED)
        assert L.dtk_debug_configure(b"BLK_SPAN", b"16") == 0
        try:
            slices = assert_offsets(st, tok, om, raw, 0, BLOCKED, blocked=False)
        finally:
            assert L.dtk_debug_configure(b"BLK_SPAN", os.environ.get("DATOK_BLK_SPAN", "-1").encode()) == 0
        assert all(sl.r_rblk is None and sl.r_rblk_head is None for sl in slices)
        for a, b in zip(slices, fit):
            assert all(np.array_equal(x, y) for x, y in zip(slice_parts(a), slice_parts(b)))
            assert a.r_carry_out == b.r_carry_out
        assert all(sl.r_blocked for sl in assert_offsets(st, tok, om, raw, 0, BLOCKED))


# ---- 12. reuse
def test_one_stream_object_through_modes(models, whole):
    import datok_amd
    from datok_amd import _lib
    from test_stream_positions import assert_positions
    from test_stream_render import assert_rendered
    tok, om = models("tokenizer_de.matok")
    raw = whole("de", "tokenizer_de.matok", om)[0]
    short = sc.running_text(30000, seed=2)
    with datok_amd.Stream(S) as st:
        # the surfaces as text and the offsets as arrays
        st.set_render(3)
        slices = assert_offsets(st, tok, om, raw, 0, BLOCKED)
        assert all(sl.out is not None and sl.written is None for sl in slices)
        assert b"".join(sl.out for sl in slices) == om.transduce(raw, 3)[0]
        with pytest.raises(_lib.DatokGpuError) as e:          # exclusive with position rendering, either way round
            st.set_position_render(15)
        assert e.value.code == _lib.E_ARG
        slices = assert_offsets(st, tok, om, short, NL, PLAIN)   # (a refused call changes nothing; a shorter stream starts fresh)
        assert all(sl.out is not None and sl.carry_out is None for sl in slices)
        assert slices[0].r_carry_in == CARRY0
        st.set_offsets(None)
        for sl in assert_rendered(st, tok, om, short, 3):
            assert sl.r_tok_rstart is None and sl.r_sent is None and sl.r_carry_out is None
        assert_positions(st, tok, om, short, 15)
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_offsets(PLAIN)
        assert e.value.code == _lib.E_ARG
        with pytest.raises(_lib.DatokGpuError) as e:
            st.set_offsets(7)
        assert e.value.code == _lib.E_ARG
        slices = assert_positions(st, tok, om, short, 28)         # (a refused call changes nothing)
        assert all(sl.r_tok_rstart is None for sl in slices)
        st.set_position_render(None)
        assert_offsets(st, tok, om, short, 0, BLOCKED)
        assert st.transduce(tok, raw, 15) == om.transduce(raw, 15)
        got = []
        st.run(tok, raw, on_slice=got.append)                     # dtk_stream_transduce leaves offset delivery off
        assert got and all(sl.r_tok_rstart is None and sl.out is None for sl in got)


# ---- 13. the literal newline rule a second time
def test_a_token_that_ends_at_zero_under_the_newline_rule_is_refused(tmp_path):
    """A crafted tokenizer (craft.matok_from) in which a newline begins a word: behind an EOT the token "\\n" has
    rstart -1 and rend 0 under NEWLINE_AFTER_EOT, so posC is 0 again at the next token, and the reference's literal
    rule (token_writer.go:51) looks at it a second time.  The run ends with DTK_E_IRREGULAR, as in position rendering."""
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
    assert 100 < len(raw) < 1000
    doc = om.transduce_doc(raw, NL)
    assert doc.status == 0 and doc.text_tok_end[0] == 3 and doc.tok_rstart[3] == -1 and doc.tok_rend[3] == 0
    with datok_amd.Stream(S) as st:
        for form in (PLAIN, BLOCKED):
            st.set_offsets(form)
            with pytest.raises(_lib.DatokGpuError) as e:
                st.run(tok, raw, flags=NL)
            assert e.value.code == _lib.E_IRREGULAR
            assert_offsets(st, tok, om, raw, 0, form)             # without the rule the same stream is regular
