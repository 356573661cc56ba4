"""The row offsets of a batch (tok_off / sent_off / text_off, the totals, n_flagged) from the scan of independent
256-document tiles, and from the three-launch scan behind it: many documents of 8..40 bytes through the public batch
API, checked against the oracle's per-document counts."""
import os

import numpy as np
import pytest

from conftest import MODELS
from parity import FIELDS, assert_batch_equals_oracle, oracle_doc

pytestmark = pytest.mark.gpu

MODEL = "tokenizer_de.matok"
N_POOL = 8193
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4096, 8191, 8192, 8193]
BLOB = b"x" * 1100          # blank-free and longer than the 1024-rune window: the document is flagged


@pytest.fixture(scope="module")
def tok():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    t = datok_amd.load_tokenizer_file(os.path.join(MODELS, MODEL))
    assert t is not None
    return t


class Oracle:
    """The oracle's answer per distinct document, computed once."""

    def __init__(self, model):
        self.model, self.cache = model, {}

    def doc(self, d: bytes):
        if d not in self.cache:
            self.cache[d] = oracle_doc(self.model, d)
        return self.cache[d]

    def counts(self, docs):
        """(tokens, sentence ints, texts, status) per document"""
        r = [self.doc(d) for d in docs]
        return (np.array([len(x["tok_rstart"]) for x in r], np.uint64), np.array([len(x["sent"]) for x in r], np.uint64),
                np.array([len(x["text_tok_end"]) for x in r], np.uint64), np.array([x["status"] for x in r], np.uint32))


@pytest.fixture(scope="module")
def oracle(oracle_models):
    return Oracle(oracle_models(MODEL))


@pytest.fixture(scope="module")
def pool():
    """N_POOL documents of 8..40 bytes: a German text cut into pieces on rune boundaries."""
    from datok_amd import corpus
    raw = corpus.german_docs(64, 4096, seed=41)[0].tobytes()
    rng = np.random.default_rng(6)
    docs, p = [], 0
    while len(docs) < N_POOL:
        q = p + int(rng.integers(8, 37))
        while (raw[q] & 0xC0) == 0x80:   # (at most three bytes further)
            q += 1
        docs.append(raw[p:q])
        p = q
    assert all(8 <= len(d) <= 40 for d in docs)
    return docs


def run(tok, docs, batch=None, chunking=None):
    import datok_amd
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    b = batch if batch is not None else datok_amd.Batch(max(len(text), 1), len(docs))
    try:
        if chunking:
            b.set_chunking(chunking[0], chunking[1], extend=0)
        b.set_input(text, off)
        b.run(tok, 0)
        return b.result(), b.totals(), text, off
    finally:
        if batch is None:
            b.close()


def excl(counts):
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64)])


def check_csr(oracle, docs, res, tot):
    nt, ns, nx, st = oracle.counts(docs)
    n = len(docs)
    for name, got, cnt, total in (("tok_off", res.tok_off, nt, tot["n_tokens"]), ("sent_off", res.sent_off, ns, tot["n_sent"]),
                                  ("text_off", res.text_off, nx, tot["n_texts"])):
        exp = excl(cnt)
        assert got.shape == (n + 1,), (name, got.shape)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (name, n, int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
        assert int(got[n]) == int(cnt.sum()) == total, (name, n, int(got[n]), int(cnt.sum()), total)
    assert np.array_equal(res.status, st), np.flatnonzero(res.status != st)[:8]
    assert tot["n_flagged"] == int(np.count_nonzero(res.status))
    assert tot["n_docs"] == n


def check_rows(oracle, docs, res):
    """every field the parity helper compares, from the cached oracle answers (documents the oracle flags: status only)"""
    exp = [oracle.doc(d) for d in docs]
    keep = [d for d, x in enumerate(exp) if x["status"] == 0]
    none = [np.zeros(0, np.int64)]
    for f in FIELDS:
        off = res.tok_off if f.startswith("tok_") else res.sent_off if f == "sent" else res.text_off
        rows = np.concatenate([np.arange(int(off[d]), int(off[d + 1]), dtype=np.int64) for d in keep] + none)
        e = np.concatenate([np.asarray(exp[d][f]).astype(np.int64) for d in keep] + none)
        assert np.array_equal(getattr(res, f)[rows].astype(np.int64), e), f


@pytest.mark.parametrize("n_docs", SIZES)
def test_exact_csr(tok, oracle, pool, n_docs):
    """The three offset arrays are the exclusive prefix sums of the oracle's per-document counts, entry [n_docs] and
    totals() are the sums: one tile, tile edges, many tiles, the last size of the one-launch scan (8192) and the first
    of the three-launch scan (8193, the same wave scan helper)."""
    docs = pool[:n_docs]
    res, tot, text, off = run(tok, docs)
    check_csr(oracle, docs, res, tot)
    check_rows(oracle, docs, res)
    step = max(1, n_docs // 64)
    assert assert_batch_equals_oracle(oracle.model, res, text, off, docs=range(0, n_docs, step)) >= min(n_docs, 64)


def test_zeros_and_edges(tok, oracle, pool):
    """Empty documents as the first and the last document of a tile, a whole tile of empty documents between two full
    ones, and a last tile that holds a single document."""
    docs = list(pool[:512]) + [b""] * 256 + list(pool[512:1025])   # tiles 0, 1 | 2: empty | 3, 4 | 5: one document
    for i in (0, 255, 1024, 1279):                                  # first and last document of tiles 0 and 4
        docs[i] = b""
    assert len(docs) == 5 * 256 + 1
    res, tot, text, off = run(tok, docs)
    check_csr(oracle, docs, res, tot)
    check_rows(oracle, docs, res)
    # (an empty document is a text without a token, flagged as by the oracle: no tokens, no sentence, one text)
    assert tot["n_flagged"] == 260
    assert np.all(res.tok_off[512:769] == res.tok_off[512]) and np.all(res.sent_off[512:769] == res.sent_off[512])
    assert res.tok_off[1281] > res.tok_off[1280] > res.tok_off[769] > res.tok_off[512] > res.tok_off[256]


def test_n_flagged(tok, oracle, pool):
    """One flagged document (a blank-free run of 1100 runes overflows the window) in the first tile, one in the middle
    tile and one in the last, among 600: n_flagged is the number of nonzero entries of status, status is the oracle's."""
    docs = list(pool[:600])
    for i in (17, 300, 599):
        docs[i] = BLOB
    res, tot, text, off = run(tok, docs)
    print("status of the flagged documents:", [int(res.status[i]) for i in (17, 300, 599)],
          "oracle:", [oracle.doc(docs[i])["status"] for i in (17, 300, 599)], "n_flagged:", tot["n_flagged"])
    assert tot["n_flagged"] == int(np.count_nonzero(res.status)) == 3
    assert np.array_equal(res.status, oracle.counts(docs)[3])
    # (behind an overflow the reference has panicked and the counts mean nothing: the other 597 rows are compared)
    assert assert_batch_equals_oracle(oracle.model, res, text, off) == 597
    for name, o, total in (("tok_off", res.tok_off, "n_tokens"), ("sent_off", res.sent_off, "n_sent"), ("text_off", res.text_off, "n_texts")):
        assert o[0] == 0 and np.all(np.diff(o.astype(np.int64)) >= 0) and int(o[600]) == tot[total], name


def test_fix_step_in_the_scan(tok, oracle, pool):
    """700 documents walked as speculative chunks of 16 bytes with no warm-up (the forcing recipe of
    test_speculative_chunks_are_exact: a good part of the lanes mispredicts): the scan kernel does the fix step of the
    first pass, the batch repairs, and the result equals the oracle in every field.  The build with the one-block
    scan repairs on this text too (repair_rounds 2 there as here, run in the same session through DATOK_GPU_LIB)."""
    docs = pool[1000:1700]
    res, tot, text, off = run(tok, docs, chunking=(16, 0))
    print("repair_rounds:", tot["repair_rounds"], "chunk_bytes:", tot["chunk_bytes"], "n_lanes:", tot["n_lanes"])
    assert tot["chunk_bytes"] == 16 and tot["repair_rounds"] >= 1
    check_csr(oracle, docs, res, tot)
    assert assert_batch_equals_oracle(oracle.model, res, text, off) == len(docs)


def test_one_batch_object_used_again(tok, oracle, pool):
    """8192, then 257, 1 and 513 documents on one batch object, each run equal to a fresh batch's: nothing stale behind
    entry [n_docs] of the earlier run is read."""
    import datok_amd
    with datok_amd.Batch(sum(len(d) for d in pool), 8192) as b:
        for n, first in ((8192, 0), (257, 3000), (1, 5000), (513, 7000)):
            docs = pool[first:first + n]
            res, tot, _, _ = run(tok, docs, batch=b)
            fresh, ftot, _, _ = run(tok, docs)
            check_csr(oracle, docs, res, tot)
            for f in ("tok_off", "sent_off", "text_off", "status") + FIELDS:
                assert np.array_equal(getattr(res, f), getattr(fresh, f)), (n, f)
            for k in ("n_tokens", "n_sent", "n_texts", "n_flagged", "n_docs"):
                assert tot[k] == ftot[k], (n, k)
