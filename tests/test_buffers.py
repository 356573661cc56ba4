"""The batch's HIP memory: every buffer that grows on demand is made to grow on a live batch, and a freed batch, model
or pipeline gives its memory back.  Results are compared with the CPU oracle throughout (tests/parity.py)."""
import os

import numpy as np
import pytest

import craft
from conftest import MODELS
from parity import FIELDS, assert_batch_equals_oracle, oracle_doc
from test_exact_and_replay import _oracle, _oracle_calls, _replayed

pytestmark = pytest.mark.gpu

TOKEN_FIELDS = ("tok_rstart", "tok_rend", "tok_bstart", "tok_bend")


def _assert_rendered(b, om, docs):
    for bits in (3, 15):
        data, o = b.render(bits)
        for d, doc in enumerate(docs):
            exp, est = om.transduce(doc, bits)
            assert est == 0 and data[int(o[d]):int(o[d + 1])] == exp, (bits, d, doc[:40])


def test_every_grown_buffer_regrows(oracle_models):
    """One batch made for 60 000 bytes of ordinary text (about 20 020 tokens, 7 524 sentence ints, 961 texts) gets
    30 000 one-letter texts: the three groups of output arrays, the renderer's workspace and output, then (16-byte
    chunks: 3 750 lanes in 59 segments) the lane and segment tables are regrown on the live object, and every result
    still equals the oracle's.  (The totals report the lanes; nothing reports the segments: that the segment tables
    hold 59 of them and the segmented compaction ran shows only in the results.)
    The device arrays of the narrow result forms follow tok_cap, which step (b) has raised for good, and tok_r16
    exists only while no document is longer than 32 767 bytes: on that batch step (d) can only make them.  A second
    batch therefore makes d_r16 and both blocked pairs at the first capacity and then gets two documents of 30 000
    bytes (30 000 tokens): all three are regrown and delivered."""
    import datok_amd
    from datok_amd import corpus
    B = datok_amd.Batch
    om = oracle_models("tokenizer_de.matok")
    tok = datok_amd.load_tokenizer_file(os.path.join(MODELS, "tokenizer_de.matok"))
    small, big = [b"Ein Baum. " * 20, b"ab"], [b"a\x04" * 30000]
    narrow = B.R_TOK_RUNE16 | B.R_TOK_RUNE_BLK | B.R_TOK_BYTE_BLK | B.R_CSR | B.R_STATUS

    def step(b, docs, fields=None, both_rune_forms=False):
        text, off = corpus.concat_docs(docs)
        b.set_result_fields(fields or B.R_ALL)
        b.set_input(text, off)
        b.run(tok, 0)
        res, tot = b.result(), b.totals()
        if fields:   # the token offsets in their narrow forms, then the same run's other arrays
            assert not len(res.tok_rstart) and not len(res.tok_bstart) and not len(res.sent)
            assert len(res.tok_bblk) == tot["n_tokens"] and (len(res.tok_r16) or len(res.tok_rblk)) == tot["n_tokens"]
            assert assert_batch_equals_oracle(om, res, text, off, fields=TOKEN_FIELDS) == len(docs)
            if both_rune_forms:   # tok_r16 came (short documents); the same run's blocked rune offsets: blk[0]
                assert len(res.tok_r16) == tot["n_tokens"] and not len(res.tok_rblk)
                b.set_result_fields(fields & ~B.R_TOK_RUNE16)
                res = b.result()
                assert len(res.tok_rblk) == tot["n_tokens"] and not len(res.tok_rstart)
                res.tok_r16 = res.tok_r16[:0]   # (BatchResult.doc decodes the blocks now)
                assert assert_batch_equals_oracle(om, res, text, off, fields=TOKEN_FIELDS) == len(docs)
            b.set_result_fields(B.R_ALL)
            res = b.result()
        assert assert_batch_equals_oracle(om, res, text, off, fields=FIELDS) == len(docs)
        _assert_rendered(b, om, docs)
        return tot

    with B(60000, 4) as b:
        step(b, small)                                            # (a) nothing grows
        for chunked in (False, True):                             # (b), (c)
            if chunked:
                b.set_chunking(16, 8)
            tot = step(b, big)
            assert (tot["n_tokens"], tot["n_sent"], tot["n_texts"], tot["n_flagged"]) == (30000, 60000, 30000, 0)
            assert not chunked or tot["n_lanes"] == 3750
        step(b, small, narrow)                                    # (d) made, then grown
        tot = step(b, big, narrow)
        assert (tot["n_tokens"], tot["n_sent"], tot["n_texts"]) == (30000, 60000, 30000)
    with B(60000, 4) as b:                                        # d_r16 and both pairs made at 20 020 tokens ...
        assert step(b, small, narrow, both_rune_forms=True)["n_tokens"] == 61
        tot = step(b, [b"a\x04" * 15000] * 2, narrow, both_rune_forms=True)   # ... and regrown
        assert (tot["n_tokens"], tot["n_sent"], tot["n_texts"]) == (30000, 60000, 30000)


def test_exact_tables_regrow(tmp_path):
    """The exact pass's tables (document ids, call counts and offsets, the calls) are sized by the run that needs them:
    a second run on the same batch that sends more than 1.25 x + 16 as many documents there regrows them."""
    import datok_amd
    from datok_amd import corpus
    blob = craft.datok()
    path = tmp_path / "crafted.datok"
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), _oracle(blob)
    docs = craft.documents(np.random.default_rng(5))
    all_text, _ = corpus.concat_docs(docs)
    n_exact = []
    with datok_amd.Batch(len(all_text), len(docs)) as b:
        for part in (docs[:16], docs):
            text, off = corpus.concat_docs(part)
            b.set_input(text, off)
            b.run(tok, 0)
            res = b.result()
            n_exact.append(len(res.exact))
            assert not any(int(s) & datok_amd.ST_IRREGULAR for s in res.status)
            in_contract = sum(1 for doc in part if oracle_doc(om, doc)["status"] == 0)
            assert assert_batch_equals_oracle(om, res, text, off) == in_contract >= 5
            for d, doc in enumerate(part):
                exp = [c[:3] if c[0] == "T" else c for c in _oracle_calls(om, doc)]
                assert _replayed(res, d, doc, False) == exp, (d, doc)
    assert n_exact[0] >= 1 and n_exact[1] > 1.25 * n_exact[0] + 16, n_exact


def test_create_and_free_return_the_memory(oracle_models):
    """Free device memory after ten create / run / result / render / free cycles of a 16 MiB batch (with a model of its
    own each) and two of a pipeline of depth 3 is within one batch's footprint F of what it was after the first cycle:
    a batch lost per cycle would be 10 F.
    Free memory is what hipMemGetInfo reports (the call behind torch.cuda.mem_get_info), asked of the HIP runtime the
    library itself runs on: torch brings a copy of the runtime of its own, and where the library's was loaded first --
    by any GPU test before this one -- torch could not open the device through its own."""
    import ctypes
    import datok_amd
    from datok_amd import corpus
    om = oracle_models("tokenizer_de.matok")
    path = os.path.join(MODELS, "tokenizer_de.matok")
    text, off = corpus.german_docs(4096, 4096, seed=2)
    n_tokens = int(om.count_batch(text, off, 4)[:, 0].sum())
    L = datok_amd.lib()

    def free_now():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert L.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    def cycle(check_docs=None):
        tok = datok_amd.load_tokenizer_file(path)
        with datok_amd.Batch(16 << 20, 4096) as b:
            b.set_input(text, off)
            b.run(tok, 0)
            res, tot = b.result(copy=False), b.totals()
            data, o = b.render(3)
            alive = free_now()
            assert tot["n_tokens"] == n_tokens and tot["n_flagged"] == 0 and int(o[-1]) == len(data) > 0
            if check_docs is not None:
                assert assert_batch_equals_oracle(om, res, text, off, docs=check_docs) == len(check_docs)
        del tok
        return alive

    def pipeline_cycle():
        tok = datok_amd.load_tokenizer_file(path)
        seen = [0]

        def on_slice(first, n, b):
            res = b.result(copy=False)
            sub_off = (off[first:first + n + 1] - off[first]).astype(np.uint64)
            assert_batch_equals_oracle(om, res, text[int(off[first]):int(off[first + n])], sub_off, docs=range(0, n, 64))
            seen[0] += b.totals()["n_tokens"]
        with datok_amd.Pipeline(4 << 20, 1024, depth=3) as p:
            p.set_result_fields(datok_amd.Batch.R_ALL)
            p.run(tok, text, off, 0, on_slice)
        assert seen[0] == n_tokens
        del tok

    free_now()
    alive = cycle(check_docs=range(0, 4096, 16))
    baseline = free_now()
    F = baseline - alive
    assert F >= 16 << 20, (baseline, alive)
    for _ in range(10):
        cycle()
    for _ in range(2):
        pipeline_cycle()
    after = free_now()
    assert abs(baseline - after) <= F, dict(baseline=baseline, alive=alive, F=F, after=after)
