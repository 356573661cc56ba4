"""The compaction (dtk_compact.hip) at its own structural edges: the lane kernel k_compact_small on the A-families of
compactedges.py, the wave kernels k_compact_plain / k_compact_eot on the B-families, every field and the rendered bytes
against the CPU oracle -- and the exact pass watched, because it repairs what a compaction kernel gets wrong:

  matrix model, no NEWLINE_AFTER_EOT   no document the oracle accepts is written by the exact pass;
  double array or NEWLINE_AFTER_EOT    the lane kernel leaves no document to the exact pass that the wave kernels keep
                                       (the walk itself hands over a double-array document whose calls leave position
                                       order, and the newline rule has a case both kernel families hand over:
                                       compactedges.exact_rule).

Every configuration runs its documents twice on fresh batches, wave kernels only (SMALL_MAX 0) and lane kernel forced,
and the rows of the two runs are equal array for array.  On the parent of the commit that added this file no family
broke the first rule: no document is excluded from it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import compactedges as ce
from compactedges import NEWLINE_AFTER_EOT, SIMPLE
from conftest import MODELS, ROOT
from parity import FIELDS

pytestmark = pytest.mark.gpu

LANE_MODELS = ["tokenizer_de.matok", "tokenizer_de.datok", "clitic_test.matok", "simpletok.datok"]
WAVE_MODELS = ["tokenizer_de.matok", "tokenizer_de.datok"]
FLAGS = [0, NEWLINE_AFTER_EOT]
ALL_BYTES = 1 << 20      # a SMALL_MAX above every document here


@pytest.fixture(scope="module")
def tok():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = datok_amd.load_tokenizer_file(os.path.join(MODELS, name))
            assert cache[name] is not None
        return cache[name]
    return get


@pytest.fixture(scope="module")
def om(oracle_models):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ce.CachedOracle(oracle_models(name))
        return cache[name]
    return get


# ------------------------------------------------------------------------------------------------ the lane kernel
@pytest.mark.parametrize("family", sorted(ce.A_FAMILIES))
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("model", LANE_MODELS)
def test_lane_kernel(tok, om, model, flags, family):
    """A1 the edge documents, A2 every length 0..160, A3 tokens over word edges, A4 EOT placements: one batch per
    family, every document through k_compact_small (SMALL_MAX 4096)."""
    docs = ce.A_FAMILIES[family]()
    assert max(len(d) for d in docs) <= 4096
    ce.check_lane_and_wave(tok(model), om(model), docs, flags, sm=4096)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("model", LANE_MODELS)
def test_lane_and_wave_kernels_write_one_set_of_arrays(tok, om, model, flags):
    """A5 under SMALL_MAX 160: documents of 159 and 160 bytes to the lane kernel, 161 and 5000 bytes to the wave kernels
    (from the list of larger documents), empty documents at both ends."""
    ce.check_lane_and_wave(tok(model), om(model), ce.a5_mixed(), flags, sm=ce.A5_SMALL_MAX)


def check_rows(om, pieces, pick, res, flags):
    """Every row of the batch against the oracle's answer per distinct piece, vectorised."""
    exp = [om.transduce_doc(p, flags) for p in pieces]
    status = np.array([exp[i].status for i in pick], np.uint32)
    assert np.array_equal(res.status, status), np.flatnonzero(res.status != status)[:8]
    keep = np.flatnonzero(status == 0)
    none = [np.zeros(0, np.int64)]
    for f in FIELDS:
        off = res.tok_off if f.startswith("tok_") else res.sent_off if f == "sent" else res.text_off
        n = np.array([len(getattr(exp[i], f)) for i in pick], np.int64)
        assert np.array_equal(np.diff(off.astype(np.int64)), n), f
        rows = np.concatenate([np.arange(int(off[d]), int(off[d + 1]), dtype=np.int64) for d in keep] + none)
        e = np.concatenate([np.asarray(getattr(exp[pick[d]], f)).astype(np.int64) for d in keep] + none)
        got = getattr(res, f)[rows].astype(np.int64)
        bad = np.flatnonzero(got != e)
        assert bad.size == 0, (f, int(rows[bad[0]]), int(got[bad[0]]), int(e[bad[0]]))
    return keep


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("model", WAVE_MODELS)
def test_lane_kernel_as_production_launches_it(tok, om, model, flags):
    """No hook: the library itself sends the small documents to k_compact_small -- dtk_run.cpp (the block that sets
    b->small_max) asks for at least LANE_MIN_DOCS = 2048 documents of which at least LANE_MIN_SMALL = 16 384 are at most
    LANE_SMALL_BYTES = 160 bytes long.  17 500 small documents from a pool of 3000 pieces (EOTs, runes of several
    bytes, every length modulo 32) among 300 larger ones, default chunking; rows, status and rendered bytes against the
    oracle, the exact pass by the rule above, and the same rows from the wave kernels alone."""
    pieces, pick = ce.production_batch()
    docs = [pieces[i] for i in pick]
    lens = np.array([len(d) for d in docs])
    assert len(docs) >= ce.LANE_MIN_DOCS and int((lens <= ce.LANE_SMALL_BYTES).sum()) >= ce.LANE_MIN_SMALL
    o = om(model)
    strict = ce.exact_rule(o.info["kind"] == 0, flags)
    with ce.ran(tok(model), docs, flags, sm=0, chunking="auto") as (b0, wave, text, off):
        check_rows(o, pieces, pick, wave, flags)
        with ce.ran(tok(model), docs, flags, sm=None, chunking="auto") as (b, res, text, off):   # (both open: see ce)
            keep = check_rows(o, pieces, pick, res, flags)
            assert len(keep) > 17000
            for bits in (SIMPLE, 15):
                data, ro = b.render(bits | flags)
                exp = [o.transduce(p, bits | flags)[0] for p in pieces]
                for d in keep:
                    assert data[int(ro[d]):int(ro[d + 1])] == exp[pick[d]], (bits | flags, int(d), docs[d][:80])
    ce.assert_same_rows(wave, res)
    exact, wave_exact = set(int(d) for d in res.exact), set(int(d) for d in wave.exact)
    if strict:
        assert not (exact & set(keep.tolist())) and not (wave_exact & set(keep.tolist()))
    else:
        assert exact <= wave_exact, sorted(exact - wave_exact)[:8]


# ------------------------------------------------------------------------------------------------ the wave kernels
@pytest.mark.parametrize("family", sorted(ce.B_FAMILIES))
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("model", WAVE_MODELS)
def test_wave_kernels(tok, om, model, flags, family):
    """B1 lengths around one and two tiles, B2 tokens across position 2048, B3 more tokens than staged rows, B4 EOTs at
    step and tile edges and around a heavy round, B5 the sentence latch: one lane per document, so one wave per document
    and no segments.  (The second run sends the same documents through the lane kernel.)"""
    ce.check_lane_and_wave(tok(model), om(model), ce.B_FAMILIES[family](), flags, sm=ALL_BYTES)


@pytest.mark.parametrize("family", ["B1", "B2", "B3", "B4"])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("model", WAVE_MODELS)
def test_wave_kernels_in_segments(tok, om, model, flags, family):
    """The same documents as chunk lanes of 32 bytes: a segment is 64 lanes, so the first segment edge falls near
    position 2048 as well and the carries come from k_seg_scan."""
    ce.check_lane_and_wave(tok(model), om(model), ce.B_FAMILIES[family](), flags, sm=ALL_BYTES, chunking=(32, 48))


_FULL_SCRIPT = r"""
import os, sys
ROOT = sys.argv[1]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import datok_amd
import compactedges as ce
from oracle import oracle as O
M = os.path.join(ROOT, "tests", "golden", "models")
for name in ("tokenizer_de.matok", "tokenizer_de.datok"):
    tok = datok_amd.load_tokenizer_file(os.path.join(M, name)); om = ce.CachedOracle(O.Model(os.path.join(M, name)))
    for flags in (0, ce.NEWLINE_AFTER_EOT):
        for family in ("B3", "B4"):
            docs = ce.B_FAMILIES[family]()
            with ce.ran(tok, docs, flags, sm=0) as (b, res, text, off):
                strict = ce.exact_rule(om.info["kind"] == 0, flags)
                n = ce.check(om, b, res, text, off, flags, expect_exact=None if strict else set(range(len(docs))))
                assert n == len(docs)
print("COMPACT FULL OK")
"""


def test_both_wave_kernels_with_every_run(tmp_path):
    """DATOK_COMPACT_FULL=1 (read once per process): k_compact_eot is launched beside k_compact_plain with the first
    run, not after the first has reported an EOT document -- B3 and B4 give the same rows."""
    script = tmp_path / "compact_full.py"
    script.write_text(_FULL_SCRIPT)
    e = dict(os.environ)
    e["DATOK_COMPACT_FULL"] = "1"
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, env=e, timeout=300)
    assert r.returncode == 0 and b"COMPACT FULL OK" in r.stdout, r.stderr.decode()[-2000:]
