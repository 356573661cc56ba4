"""The symboliser against its reference (tests/symref.py) on the edges of a kernel that decodes in registers
(tests/symlanes.py): every sequence at every residue of a lane, a row of lanes, a half-wave and a wave; document
boundaries and empty documents at every byte of a lane and around a block's first byte; lanes with unequal numbers of
lead bytes and sequences that cover the next lane's, wave's and block's first bytes; batches of a few bytes and of a
KiB more or less, from the host and from device pointers 0..3 bytes off; and one batch object used again after each
of them.  One-byte codes (a shipped model) and 16-bit entries (the crafted one): the two kernels see the same input.
Bit exact; nothing is excluded."""
import os
import subprocess
import sys

import numpy as np
import pytest

import symlanes
import symref
from conftest import ROOT
from symgpu import CRAFTED, SHIPPED, Ctx, run_batch, same_results, same_stream

pytestmark = pytest.mark.gpu
MODELS = [SHIPPED[0], CRAFTED]
BIG = ("lane edges", "lane cuts", "block cuts", "uneven loops", "uneven loops, cut")


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    return Ctx(tmp_path_factory.mktemp("symlanes"))


@pytest.fixture(scope="module")
def batches():
    """name -> (text, doc_off), built once (without a model's extra sequences: the same bytes for both models)."""
    return {name: (text, off) for name, text, off in symlanes.corpora()}


def _check(ctx, name, key, text, off):
    tok = ctx.model(name)[0]
    with run_batch(tok, text, off) as b:
        symref.assert_stream_equal(b.debug_stream(), ctx.ref(name, key, text, off), text, off, "%s (%s)" % (name, key))


@pytest.mark.parametrize("name", MODELS)
def test_every_lane_edge(ctx, batches, name):
    """symlanes.lane_edges: before, across at every split and behind every 8-, 16-, 32- and 64-byte edge inside a
    wave, over every KiB boundary and counted from it (the halo words of a wave's first and last lane), inside one
    document."""
    text, off = batches["lane edges"]
    assert len(text) >= len(symref.sequences()) * 64 * symlanes.ROW
    _check(ctx, name, "lane edges", text, off)


@pytest.mark.parametrize("key", ["lane cuts", "block cuts"])
@pytest.mark.parametrize("name", MODELS)
def test_document_boundaries_inside_a_lane(ctx, batches, name, key):
    """symlanes.lane_cuts and block_cuts: a boundary, one empty document and 70 of them at every byte offset 0..16 of
    the lane that holds a sequence, and around a block's first byte with the sequence across it."""
    text, off = batches[key]
    lens = np.diff(off.astype(np.int64))
    assert (lens == 0).sum() >= (1 + 70) * 17 and lens.min() == 0
    _check(ctx, name, key, text, off)


@pytest.mark.parametrize("key", ["uneven loops", "uneven loops, cut"])
@pytest.mark.parametrize("name", MODELS)
def test_uneven_loops_and_spills(ctx, batches, name, key):
    """symlanes.uneven_loops: lanes of a wave with 0 .. 16 lead bytes in rising and falling order, stray continuation
    bytes, and sequences that cover the first bytes of the next lane, wave and block."""
    text, off = batches[key]
    _check(ctx, name, key, text, off)


@pytest.mark.parametrize("name", MODELS)
def test_small_batches(ctx, name):
    """1..80 bytes and 1024 -17..+17 bytes, 0x80 first and a truncated e2 82 last: the ragged store, lanes and waves
    without input, a last word of fewer than four bytes."""
    tok = ctx.model(name)[0]
    for n in symlanes.SMALL:
        text, off = symlanes.small(n)
        with run_batch(tok, text, off) as b:
            ref = ctx.ref(name, "small%d" % n, text, off)
            assert ref[2]
            symref.assert_stream_equal(b.debug_stream(), ref, text, off, "%s (%d bytes)" % (name, n))


@pytest.mark.parametrize("name", MODELS)
def test_the_batch_used_again_after_each(ctx, batches, name):
    """One batch object of the largest size takes every batch above in turn, the small ones shared out between the
    large: stream, flag, results and all five event bitmaps equal a fresh batch's.  Both kernels carry the clears."""
    import datok_amd
    tok = ctx.model(name)[0]
    share = -(-len(symlanes.SMALL) // len(BIG))
    steps = []
    for i, key in enumerate(BIG):
        steps.append((key,) + batches[key])
        steps += [("small%d" % n,) + symlanes.small(n) for n in symlanes.SMALL[share * i:share * (i + 1)]]
    assert len(steps) == len(BIG) + len(symlanes.SMALL)
    with datok_amd.Batch(max(len(t) for _, t, _ in steps), max(len(o) - 1 for _, _, o in steps)) as b:
        for key, text, off in steps:
            b.set_input(text, off)
            b.run(tok, 0)
            res, stream = b.result(), b.debug_stream()
            symref.assert_stream_equal(stream, ctx.ref(name, key, text, off), text, off, "%s used again: %s" % (name, key))
            with run_batch(tok, text, off) as fresh:
                rf = fresh.result()
                same_stream(stream, fresh.debug_stream(), key)
                same_results(res, rf, key)
                assert res.ev_bits.shape == rf.ev_bits.shape and res.ev_bits.shape[0] == 5, key
                assert np.array_equal(res.ev_bits, rf.ev_bits), (key, np.flatnonzero((res.ev_bits != rf.ev_bits).any(axis=0))[:8])


_DEVICE_SCRIPT = r"""
import os, sys, tempfile
ROOT, name, k = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
torch.cuda.set_device(0)                  # torch's runtime first (tests/symgpu.py)
torch.cuda.synchronize()
import symgpu, symlanes
with tempfile.TemporaryDirectory() as tmp:
    ctx = symgpu.Ctx(tmp)
    for n in symlanes.SMALL:
        text, off = symlanes.small(n)
        symgpu._device_equals_host_and_reference(ctx, name, "small%d" % n, text, off, k)
    del ctx
print("DEVICE OK", name, k)
"""


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("name", MODELS)
def test_small_batches_from_device_pointers(tmp_path, name, k):
    """The same small batches in exactly sized device tensors, from a pointer k bytes off a 4-byte boundary: stream,
    bitmap, flag, offsets and rendering equal the reference and the same text sent through set_input.  (A fresh child,
    where torch opens the device before the library is loaded: symgpu's device cases.)"""
    script = tmp_path / "small_device.py"
    script.write_text(_DEVICE_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT, name, str(k)], capture_output=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and b"DEVICE OK" in r.stdout, (r.stdout.decode()[-1000:], r.stderr.decode()[-3000:])
