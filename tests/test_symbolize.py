"""k_symbolize against its reference (tests/symref.py): the symbol stream, the rune-start bitmap and the "saw an
invalid byte" flag at every byte of batches that put every kind of UTF-8 sequence on the kernel's structural edges --
tile, quarter, block and halo, document boundaries, the document table in LDS and in memory, the sigma in LDS and in
memory, full and ragged stores, one-byte codes and 16-bit entries --, the clears that ride on the kernel when a batch
is used again, and device-resident input (dtk_batch_set_input_device: the byte-wise loads for a caller's buffer that
is not aligned or not padded), accepted and rejected.  Bit exact; nothing is excluded."""
import os
import subprocess
import sys

import numpy as np
import pytest

import symref
from conftest import ROOT
from parity import assert_batch_equals_oracle
from symgpu import CRAFTED, SHIPPED, SIMPLE, ST_EMPTY_TEXT, Ctx, rows_batch, run_batch, same_results

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    return Ctx(tmp_path_factory.mktemp("sym"))


# ---------------------------------------------------------------- stream, bitmap and flag against the reference
def test_accessor_needs_a_run(ctx):
    import datok_amd
    tok = ctx.model(SHIPPED[0])[0]
    text, off = symref.tail(33)
    with datok_amd.Batch(64, 4) as b:
        for step in ("fresh", "input set"):
            with pytest.raises(datok_amd.DatokGpuError) as e:
                b.debug_stream()
            assert e.value.code == datok_amd._lib.E_ARG, step
            b.set_input(text, off)
        b.run(tok, 0)
        assert len(b.debug_stream()[0]) == 33
        b.set_input(text, off)               # a new input: the stream on the device belongs to no run of it
        with pytest.raises(datok_amd.DatokGpuError):
            b.debug_stream()


@pytest.mark.parametrize("lay", ["a", "b", "c", "c@8192", "c@row1"])
@pytest.mark.parametrize("name", SHIPPED + [CRAFTED])
def test_stream_of_the_rows(ctx, name, lay):
    """Every sequence at every split across a tile, quarter and block edge: (a) inside one document, (b) cut by a
    document boundary at the edge, (c) in documents of 8 bytes -- 512 per block, so the kernel searches the offsets in
    memory --, and (c) again with a sequence's first byte as byte 0 of the batch."""
    tok = ctx.model(name)[0]
    key, text, off = rows_batch(ctx, name, lay)
    assert len(text) > 100 * symref.ROW
    with run_batch(tok, text, off) as b:
        symref.assert_stream_equal(b.debug_stream(), ctx.ref(name, key, text, off), text, off, "%s (%s)" % (name, lay))


@pytest.mark.parametrize("name", SHIPPED + [CRAFTED])
def test_stream_of_the_tails(ctx, name):
    """The ragged store path, a last tile of fewer than 8 bytes per lane, a last block shorter than a quarter."""
    tok = ctx.model(name)[0]
    for n in symref.TAILS:
        text, off = symref.tail(n)
        with run_batch(tok, text, off) as b:
            got, ref = b.debug_stream(), ctx.ref(name, "tail%d" % n, text, off)
            assert ref[2]
            symref.assert_stream_equal(got, ref, text, off, "%s (tail of %d bytes)" % (name, n))


@pytest.mark.parametrize("name", SHIPPED + [CRAFTED])
def test_stream_of_full_queues(ctx, name):
    """Quarters whose every byte is queued (1024 entries): 512 two-byte runes, 1024 stray continuation bytes, 4096
    invalid bytes, on a quarter edge and one byte behind it.  (Stream only: these documents overflow the reference's
    window of 1024 runes by design.)"""
    tok = ctx.model(name)[0]
    text, off = symref.dense()
    with run_batch(tok, text, off) as b:
        symref.assert_stream_equal(b.debug_stream(), ctx.ref(name, "dense", text, off), text, off, name + " (dense)")


_SYM16_SCRIPT = r"""
import os, sys
ROOT = sys.argv[1]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datok_amd
import symref
from oracle import oracle as O
M = os.path.join(ROOT, "tests", "golden", "models")
text, what = symref.rows()
off = symref.layout(len(what), "a")
for name in ("tokenizer_de.matok", "tokenizer_de.datok"):
    tok, om = datok_amd.load_tokenizer_file(os.path.join(M, name)), O.Model(os.path.join(M, name))
    assert tok.info["stream_codes"] == 0, tok.info
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_input(text, off); b.run(tok, 0)
        symref.assert_stream_equal(b.debug_stream(), symref.reference_stream(om, text, off), text, off, name + " (16-bit entries)")
        assert not b.result().status.any()
print("SYM16 OK")
"""


def test_stream_of_16_bit_entries_with_the_sigma_in_lds(tmp_path):
    """DATOK_SYM16=1 makes a shipped model's stream hold the 16-bit entries: the instantiation the crafted model takes,
    but with the sigma's runes in LDS.  The environment is forwarded to the library once, when a process first loads it,
    so a switch set here reaches a fresh child only.  (The hook behind the switch is read at every model load: set through
    dtk_debug_configure around one load, it gives that model the same stream in this process -- bigsigma.device_model.)"""
    script = tmp_path / "sym16.py"
    script.write_text(_SYM16_SCRIPT)
    e = dict(os.environ); e["DATOK_SYM16"] = "1"
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, env=e, timeout=600)
    assert r.returncode == 0 and b"SYM16 OK" in r.stdout, (r.stdout.decode()[-500:], r.stderr.decode()[-2000:])


# ---------------------------------------------------------------- end to end on the same batches
C_PARTS = 4     # layout (c) has 240 000 documents: compared in four parts, a few seconds each


@pytest.mark.parametrize("case", ["a", "b"] + ["c/%d" % k for k in range(C_PARTS)])
@pytest.mark.parametrize("name", SHIPPED)
def test_offsets_and_rendering_of_the_rows(ctx, name, case):
    """Token offsets of every document against the oracle, and the SIMPLE rendering against the oracle's bytes: an
    invalid byte prints as U+FFFD, which takes the stream's widths and the flag.  The oracle finishes every document
    (status 0), but for the ten of (b) and of (c) that begin with U+0004 -- the `e28204` and `f09f9804` rows at the
    split that puts the EOT first: an empty text, ST_EMPTY_TEXT; they are counted.  (Every offset of (c) is a
    multiple of 8 and so is every B: the same ten bytes begin a document in (b) and in (c).)"""
    tok, _, memo, _ = ctx.model(name)
    lay = case[0]
    _, text, off = rows_batch(ctx, name, lay)
    n = len(off) - 1
    docs = range(n) if lay != "c" else range(int(case[2:]) * n // C_PARTS, (int(case[2:]) + 1) * n // C_PARTS)
    raw = text.tobytes()
    flagged = [d for d in docs if memo.transduce_doc(raw[int(off[d]):int(off[d + 1])], 0).status]
    for d in flagged:
        assert raw[int(off[d])] == 4 and memo.transduce_doc(raw[int(off[d]):int(off[d + 1])], 0).status == ST_EMPTY_TEXT, d
    if lay == "a":
        assert not flagged
    elif lay == "b" or case == "c/0":
        every = [d for d in range(n) if memo.transduce_doc(raw[int(off[d]):int(off[d + 1])], 0).status]
        assert len(every) == 10 and all(raw[int(off[d])] == 4 for d in every), every
    with run_batch(tok, text, off) as b:
        res = b.result()
        assert assert_batch_equals_oracle(memo, res, text, off, docs=docs) == len(docs) - len(flagged)
        data, o = b.render(SIMPLE)
        for d in docs:
            exp, est = memo.transduce(raw[int(off[d]):int(off[d + 1])], SIMPLE)
            assert est == 0 and data[int(o[d]):int(o[d + 1])] == exp, (case, d, raw[int(off[d]):int(off[d + 1])][:40])


# ---------------------------------------------------------------- reuse: the clears that ride on k_symbolize
def test_a_batch_used_again_starts_from_clean_bitmaps_and_flag(ctx):
    """k_symbolize's blocks clear the event bitmaps and the accumulator block, and the flag is the number of the last
    run that saw an invalid byte.  One batch takes, in turn: 240 000 tiny documents with invalid bytes; a short clean
    text; runs of 70 and 4100 empty documents around every block boundary and at both ends; one document per row.
    After each run everything equals the reference and a fresh batch given the same input -- all words of the five
    event bitmaps included."""
    import datok_amd
    name = SHIPPED[0]
    tok, _, memo, _ = ctx.model(name)
    _, text, off_c = rows_batch(ctx, name, "c")
    _, _, off_a = rows_batch(ctx, name, "a")
    short = np.frombuffer(symref.filler(700), dtype=np.uint8).copy()
    steps = [("c", text, off_c, True, range(0, len(off_c) - 1, 16)),
             ("short", short, np.array([0, 300, 700], dtype=np.uint64), False, None),
             ("empty runs",) + symref.empty_runs() + (False, None),
             ("a", text, off_a, True, None)]
    with datok_amd.Batch(len(text), len(off_c) - 1) as b:
        for key, t, off, invalid, docs in steps:
            b.set_input(t, off)
            b.run(tok, 0)
            res, stream = b.result(), b.debug_stream()
            ref = ctx.ref(name, key, t, off)
            assert ref[2] == invalid and stream[2] == invalid, key
            symref.assert_stream_equal(stream, ref, t, off, "used again: " + key)
            with run_batch(tok, t, off) as fresh:
                rf = fresh.result()
                same_results(res, rf, key)
                assert res.ev_bits.shape == rf.ev_bits.shape and res.ev_bits.shape[0] == 5, key
                assert np.array_equal(res.ev_bits, rf.ev_bits), (key, np.flatnonzero((res.ev_bits != rf.ev_bits).any(axis=0))[:8])
            # the offsets against the oracle: every document; of the 240 000 of (c) every sixteenth here (all of them
            # in test_offsets_and_rendering_of_the_rows, whose batch the fresh one above repeats)
            checked = assert_batch_equals_oracle(memo, res, t, off, docs=docs)
            assert checked > 0


# ---------------------------------------------------------------- device-resident input
def _child(*args):
    """A case of tests/symgpu.py in a fresh process, where torch opens the device before the library is loaded."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "symgpu.py")] + [str(a) for a in args],
                       capture_output=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and b"DEVICE OK" in r.stdout, (r.stdout.decode()[-1000:], r.stderr.decode()[-3000:])


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("name", [SHIPPED[0], CRAFTED])
def test_device_resident_input(name, k):
    """bench.py's path (symgpu.resident).  A caller's buffer is read with 4-byte loads only if its address and its
    size are multiples of 4 (k_symbolize<true, *> on a buffer without padding), else byte by byte (<false, *>):
    torch tensors sliced 0..3 bytes off, sizes of every residue, exactly sized; layouts (a) and (c) and the tails,
    codes and 16-bit entries.  Stream, bitmap, flag, offsets and rendering equal the reference, and -- bit for bit --
    the same text sent through set_input on another batch."""
    _child("resident", name, k)


@pytest.mark.parametrize("name", [SHIPPED[0], CRAFTED])
def test_host_device_host_input_with_the_same_offsets(name):
    """symgpu.alternate: one batch, host, device and host input with identical offsets, twice over; every run exact,
    whether the lane plan is kept (host after host) or made anew (the offsets live in another buffer)."""
    _child("alternate", name)


@pytest.mark.parametrize("previous", ["host", "device"])
def test_rejected_device_input_leaves_the_batch_as_it_was(previous):
    """symgpu.rejected: doc_off[0] != 0, doc_off[n] != total, a decreasing pair, n_docs > max_docs, total > max_bytes
    -- each is refused with DTK_E_ARG or DTK_E_CAPACITY, and the run that follows reproduces the previous input's
    stream, offsets, bitmaps and rendering exactly."""
    _child("rejected", previous)
