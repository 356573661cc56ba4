"""Token offsets as 16-bit blocks (DTK_R_TOK_RUNE_BLK / DTK_R_TOK_BYTE_BLK, include/datok_gpu.h): 4.25 B per token on
the link for documents of any length.

CPU tier: the numpy encoder of tests/blocked.py (written from the format's description) against the two decoders
(datok_amd.unpack_blocked; dtk_blk_start / dtk_blk_end compiled as C), on the oracle's offsets.
GPU tier: k_pack_blk and the download path -- the delivered words and headers equal, word for word and header for
header, the encoder applied to the 32-bit arrays of the same run (a second download), and the oracle.
"""
import os
import subprocess

import numpy as np
import pytest

import blocked
import craft
from conftest import MODELS, ROOT
from parity import assert_batch_equals_oracle

NEWLINE_AFTER_EOT, OFFSETS_ONLY, NO_BYTE_OFFSETS, NO_RUNE_OFFSETS = 16, 256, 512, 1024
MODELS_DE = ("tokenizer_de.matok", "tokenizer_de.datok")
PAIRS = (("tok_rstart", "tok_rend"), ("tok_bstart", "tok_bend"))


def _five(oracle_models, model, flags):
    docs = blocked.five_documents()
    return docs, blocked.oracle_batch(oracle_models(model), ("five", model, flags), docs, flags)


# ---------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("flags", [0, NEWLINE_AFTER_EOT])
@pytest.mark.parametrize("model", MODELS_DE)
def test_encoder_round_trip_on_the_oracles_offsets(oracle_models, model, flags):
    """encode -> unpack_blocked gives the offsets back; no block of the five-document batch overflows 16 bits
    (the span limit of 65 535), and blocks do overflow at a span limit of 255."""
    import datok_amd
    docs, exp = _five(oracle_models, model, flags)
    assert [len(d) for d in docs][:3] == [100000, 9, 100000] and len(docs[3]) > 204000 and not exp["status"].any()
    assert int(exp["tok_off"][5] - exp["tok_off"][4]) == 71       # the tokens of 1000 bytes
    for fs, fe in PAIRS:
        words, heads, overflow, worst = blocked.encode(exp[fs], exp[fe])
        assert overflow == 0 and 1000 < worst <= 65535, (fs, worst)
        assert words.dtype == np.uint32 and heads.shape == ((len(words) + 63) // 64, 4) and not heads[:, 3].any()
        s, e = datok_amd.unpack_blocked(words, heads)
        assert s.dtype == np.int32 and np.array_equal(s, exp[fs].astype(np.int32)) and np.array_equal(e, exp[fe].astype(np.int32))
        a, b = int(exp["tok_off"][3]), int(exp["tok_off"][4])     # (a range of tokens: what BatchResult.doc decodes)
        s, e = datok_amd.unpack_blocked(words, heads, a, b)
        assert np.array_equal(s, exp[fs][a:b].astype(np.int32)) and np.array_equal(e, exp[fe][a:b].astype(np.int32))
        assert blocked.encode(exp[fs], exp[fe], span=255)[2] > 0
    # the document boundaries and the two EOTs are breaks
    _, heads, _, _ = blocked.encode(exp["tok_rstart"], exp["tok_rend"])
    assert int((heads[:, 2] < 64).sum()) >= 4


def test_c_decoders_equal_numpy(oracle_models, tmp_path):
    """dtk_blk_start / dtk_blk_end of include/datok_gpu.h, compiled as C99 by the host compiler."""
    docs, exp = _five(oracle_models, MODELS_DE[0], 0)
    words, heads, _, _ = blocked.encode(exp["tok_rstart"], exp["tok_rend"])
    src = tmp_path / "decode.c"
    src.write_text(r'''
#include <stdio.h>
#include <stdlib.h>
#include "datok_gpu.h"
int main(int argc, char **argv) {
  size_t n = (size_t)atol(argv[1]), nb = (n + 63) / 64, i;
  uint32_t *w = malloc(n * 4 + 4);
  dtk_off_block *h = malloc(nb * sizeof *h + 16);
  int32_t *out = malloc(n * 8 + 8);
  FILE *f = fopen(argv[2], "rb"), *g;
  if (sizeof(dtk_off_block) != 16 || !f || fread(w, 4, n, f) != n || fread(h, sizeof *h, nb, f) != nb) return 1;
  for (i = 0; i < n; i++) { out[2 * i] = dtk_blk_start(w, h, i); out[2 * i + 1] = dtk_blk_end(w, h, i); }
  g = fopen(argv[3], "wb");
  return !g || fwrite(out, 8, n, g) != n || fclose(g) != 0;
}
''')
    exe, inp, outp = tmp_path / "decode", tmp_path / "in.bin", tmp_path / "out.bin"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    inp.write_bytes(words.tobytes() + heads.tobytes())
    subprocess.check_call([str(exe), str(len(words)), str(inp), str(outp)])
    got = np.frombuffer(outp.read_bytes(), dtype=np.int32).reshape(-1, 2)
    assert np.array_equal(got[:, 0], exp["tok_rstart"]) and np.array_equal(got[:, 1], exp["tok_rend"])
    # the same two functions as the library exports them (for callers that bind symbols)
    import datok_amd
    L = datok_amd.lib()
    for i in (0, 63, 64, len(words) // 2, len(words) - 1):
        assert L.dtk_blk_start(words.ctypes.data, heads.ctypes.data, i) == int(exp["tok_rstart"][i])
        assert L.dtk_blk_end(words.ctypes.data, heads.ctypes.data, i) == int(exp["tok_rend"][i])


# ---------------------------------------------------------------------------------------------------- GPU tier
@pytest.fixture(scope="module")
def gpu():
    import datok_amd
    assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = datok_amd.load_tokenizer_file(os.path.join(MODELS, name))
            assert cache[name] is not None
        return cache[name]
    return get


def _B():
    import datok_amd
    return datok_amd.Batch


def _both():
    return _B().R_TOK_RUNE_BLK | _B().R_TOK_BYTE_BLK


def _blocked_result(b, fields, pairs=(0, 1)):
    """result() with `fields`, then the 32-bit arrays of the same run by a second download: the blocked arrays of
    `pairs` are there and equal the numpy encoder on the 32-bit arrays, the other pairs' are absent.  Returns both."""
    B = _B()
    b.set_result_fields(fields)
    r = b.result()
    n = b.totals()["n_tokens"]
    for k, (words, heads) in enumerate(((r.tok_rblk, r.tok_rblk_head), (r.tok_bblk, r.tok_bblk_head))):
        assert (len(words), len(heads)) == ((n, (n + 63) // 64) if k in pairs else (0, 0)), (k, len(words), len(heads), n)
    wide = B.R_TOK_RUNE * (0 in pairs) | B.R_TOK_BYTE * (1 in pairs)
    b.set_result_fields(fields | wide)
    r32 = b.result()
    for k in pairs:
        s, e = getattr(r32, PAIRS[k][0]), getattr(r32, PAIRS[k][1])
        assert len(s) == n and len(e) == n
        words, heads, overflow, _ = blocked.encode(s, e)
        assert overflow == 0
        got_w, got_h = (r.tok_rblk, r.tok_rblk_head) if k == 0 else (r.tok_bblk, r.tok_bblk_head)
        assert np.array_equal(got_h, heads), (k, np.flatnonzero((got_h != heads).any(axis=1))[:4])
        assert np.array_equal(got_w, words), (k, np.flatnonzero(got_w != words)[:4])
    b.set_result_fields(fields)
    return r, r32


def _run(tok, docs, fields, flags=0, pairs=(0, 1), om=None):
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    with _B()(max(len(text), 1), len(docs)) as b:
        b.set_input(text, off)
        b.run(tok, flags)
        r, r32 = _blocked_result(b, fields, pairs)
        if om is not None:   # (BatchResult.doc decodes the blocks where the 32-bit arrays are absent)
            names = [f for k in pairs for f in PAIRS[k]]
            assert len(r.tok_rstart) == 0 and len(r.tok_bstart) == 0
            assert assert_batch_equals_oracle(om, r, text, off, flags & NEWLINE_AFTER_EOT, fields=names) > 0
        return r, r32, b.totals()


@pytest.mark.gpu
def test_partial_last_block(gpu, oracle_models):
    """1 ... 129 tokens: lanes behind the last token take part in nothing; no token: no launch, empty arrays."""
    B = _B()
    tok, om = gpu(MODELS_DE[0]), oracle_models(MODELS_DE[0])
    fields = _both() | B.R_CSR | B.R_STATUS
    for n in (1, 63, 64, 65, 128, 129):
        r, _, tot = _run(tok, [b" ".join(bytes([97 + k % 26]) for k in range(n))], fields, om=om)
        assert tot["n_tokens"] == n and len(r.tok_rblk_head) == (n + 63) // 64
        assert int(r.tok_rblk_head[-1, 2]) == 64 and int(r.tok_rblk_head[0, 0]) in (-1, 0)
    r, _, tot = _run(tok, [b"   \n  "], fields)
    assert tot["n_tokens"] == 0 and len(r.tok_rblk) == 0 and len(r.tok_bblk_head) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, NEWLINE_AFTER_EOT])
@pytest.mark.parametrize("model", MODELS_DE)
def test_five_document_batch(gpu, oracle_models, model, flags):
    """Long running text, a tiny document, a document of three texts, tokens of 1000 bytes: the blocked pointers are
    delivered, the 32-bit arrays and tok_r16 are absent, and everything equals the oracle."""
    B = _B()
    docs, exp = _five(oracle_models, model, flags)
    r, r32, tot = _run(gpu(model), docs, _both() | B.R_CSR | B.R_STATUS, flags)
    assert len(r.tok_rstart) == 0 and len(r.tok_bstart) == 0 and len(r.tok_r16) == 0
    assert np.array_equal(r.tok_off, exp["tok_off"]) and not r.status.any()
    for f in (f for p in PAIRS for f in p):
        assert np.array_equal(getattr(r32, f), exp[f]), f
    import datok_amd
    s, e = datok_amd.unpack_blocked(r.tok_rblk, r.tok_rblk_head)
    assert np.array_equal(s, exp["tok_rstart"]) and np.array_equal(e, exp["tok_rend"])
    got = r.doc(3)
    assert np.array_equal(got["tok_bend"], exp["tok_bend"][int(exp["tok_off"][3]):int(exp["tok_off"][4])])


@pytest.mark.gpu
@pytest.mark.parametrize("lane", [0, 1, 63])
def test_document_boundary_at_lane(gpu, oracle_models, lane):
    """A first document of more than 65 535 runes whose token count puts the next document's first token at lane 0, 1
    and 63 of a block (lane 0 has no predecessor in its block: no break there)."""
    B = _B()
    tok, om = gpu(MODELS_DE[0]), oracle_models(MODELS_DE[0])
    n1 = 344 * 64 + lane
    docs = [b"ab " * n1, b"Der Baum ist gr\xc3\xbcn. " * 40]
    r, r32, tot = _run(tok, docs, _both() | B.R_CSR | B.R_STATUS, om=om)
    assert int(r.tok_off[1]) == n1 and int(r32.tok_rend[n1 - 1]) > 65535
    head = r.tok_rblk_head[n1 // 64]
    assert int(head[2]) == (lane if lane else 64) and (not lane or int(head[0]) == int(r32.tok_rstart[n1 - lane]) > 65535)


@pytest.mark.gpu
def test_two_resets_in_one_block(gpu, oracle_models):
    """long -> 3-token document -> long: one block holds two resets, its second segment both of the short documents'."""
    B = _B()
    tok, om = gpu(MODELS_DE[1]), oracle_models(MODELS_DE[1])
    n1 = 344 * 64 + 10
    r, r32, tot = _run(tok, [b"ab " * n1, b"ab cd ef", b"xy " * 23000], _both() | B.R_CSR | B.R_STATUS, om=om)
    assert [int(x) for x in r.tok_off] == [0, n1, n1 + 3, n1 + 3 + 23000]
    assert int(r.tok_bblk_head[344, 2]) == 10 and int(r.tok_bblk_head[344, 1]) == 0 and int(r.tok_bblk_head[344, 0]) > 65535


@pytest.mark.gpu
def test_fallback_to_the_32_bit_arrays(gpu, oracle_models):
    """BLK_SPAN=255: blocks of the five-document batch do not fit, the blocked pointers are NULL and the 32-bit arrays
    are delivered in their place; a second result() returns the same; R_TOK_RUNE16 does not look at the hook."""
    import datok_amd
    from datok_amd import corpus
    B = _B()
    model = MODELS_DE[0]
    docs, exp = _five(oracle_models, model, 0)
    text, off = corpus.concat_docs(docs)
    short = corpus.german_docs(16, 2048, seed=3)
    assert datok_amd.lib().dtk_debug_configure(b"BLK_SPAN", b"255") == 0
    try:
        with B(len(text), len(docs)) as b:
            b.set_input(text, off)
            b.set_result_fields(_both() | B.R_CSR | B.R_STATUS)
            b.run(gpu(model), 0)
            for _ in range(2):
                r = b.result()
                assert len(r.tok_rblk) == 0 and len(r.tok_rblk_head) == 0 and len(r.tok_bblk) == 0 and len(r.tok_bblk_head) == 0
                for f in (f for p in PAIRS for f in p):
                    assert np.array_equal(getattr(r, f), exp[f]), f
            b.run(gpu(model), NO_BYTE_OFFSETS | OFFSETS_ONLY)       # (the next run: packed, flagged and replaced again)
            r = b.result()
            assert len(r.tok_rblk) == 0 and np.array_equal(r.tok_rstart, exp["tok_rstart"]) and len(r.tok_bstart) == 0
        with B(len(short[0]), 16) as b:
            b.set_input(*short)
            b.set_result_fields(B.R_TOK_RUNE16 | B.R_CSR | B.R_STATUS)
            b.run(gpu(model), 0)
            r = b.result()
            assert len(r.tok_r16) == b.totals()["n_tokens"] and len(r.tok_rstart) == 0
            assert_batch_equals_oracle(oracle_models(model), r, short[0], short[1], fields=("tok_rstart", "tok_rend"))
    finally:
        assert datok_amd.lib().dtk_debug_configure(b"BLK_SPAN", b"-1") == 0
    r, _, _ = _run(gpu(model), docs[3:], _both() | B.R_CSR | B.R_STATUS)   # (the default span is back)
    assert len(r.tok_rblk) == int(exp["tok_off"][5] - exp["tok_off"][3])


@pytest.mark.gpu
def test_narrowest_form_that_applies(gpu, oracle_models):
    """R_TOK_RUNE16 | R_TOK_RUNE_BLK: a batch of 4 KiB documents gets tok_r16, the same batch plus one document of
    40 KB the blocked form."""
    from datok_amd import corpus
    B = _B()
    tok, om = gpu(MODELS_DE[0]), oracle_models(MODELS_DE[0])
    t, o = corpus.german_docs(12, 4096, seed=17)
    docs = [t[int(o[d]):int(o[d + 1])].tobytes() for d in range(12)]
    fields = B.R_TOK_RUNE16 | B.R_TOK_RUNE_BLK | B.R_CSR | B.R_STATUS
    with B(len(t), 12) as b:
        b.set_input(t, o)
        b.set_result_fields(fields)
        b.run(tok, 0)
        for _ in range(2):
            r = b.result()
            assert len(r.tok_r16) == b.totals()["n_tokens"] and len(r.tok_rblk) == 0 and len(r.tok_rstart) == 0
        assert_batch_equals_oracle(om, r, t, o, fields=("tok_rstart", "tok_rend"))
    r, _, _ = _run(tok, docs + [b"".join(docs[:10])[:40000]], fields, pairs=(0,), om=om)
    assert len(r.tok_r16) == 0


@pytest.mark.gpu
def test_one_batch_long_short_long(gpu, oracle_models):
    """One batch object, long -> short -> long with growing token counts (the third run outgrows the token arrays the
    batch was created with): no stale flag, header or capacity."""
    import datok_amd
    from datok_amd import corpus
    B = _B()
    tok, om = gpu(MODELS_DE[0]), oracle_models(MODELS_DE[0])
    t, o = corpus.german_docs(2, 70000, seed=19)
    inputs = [(t, o), corpus.concat_docs([b"Ein Baum. " * 20, b"ab"]),
              corpus.concat_docs([b"a " * 69000, b"b c " * 200])]
    fields = _both() | B.R_CSR | B.R_STATUS
    assert datok_amd.lib().dtk_debug_configure(b"BLK_SPAN", b"255") == 0
    try:
        with B(140000, 4) as b:
            n_before = 0
            for k, (text, off) in enumerate(inputs):
                if k == 1:
                    assert datok_amd.lib().dtk_debug_configure(b"BLK_SPAN", b"0") == 0
                b.set_input(text, off)
                b.run(tok, 0)
                if k == 0:      # (the first run falls back: its raised flag must not reach the next runs)
                    b.set_result_fields(fields)
                    r = b.result()
                    assert len(r.tok_rblk) == 0 and len(r.tok_bblk) == 0 and len(r.tok_rstart) == b.totals()["n_tokens"]
                else:
                    r, _ = _blocked_result(b, fields)
                    assert len(r.tok_rstart) == 0
                assert_batch_equals_oracle(om, r, text, off, fields=[f for p in PAIRS for f in p])
                n = b.totals()["n_tokens"]
                assert k != 2 or n > max(n_before, 140000 // 3 + 4 + 16)
                n_before = max(n_before, n)
    finally:
        assert datok_amd.lib().dtk_debug_configure(b"BLK_SPAN", b"-1") == 0


@pytest.mark.gpu
def test_no_rune_offsets_leaves_the_byte_pair(gpu, oracle_models):
    """DTK_NO_RUNE_OFFSETS masks DTK_R_TOK_RUNE_BLK as it masks DTK_R_TOK_RUNE: only the byte pair arrives."""
    B = _B()
    docs = [b"ab " * 23000, b"Ein Baum. " * 30]
    r, _, _ = _run(gpu(MODELS_DE[0]), docs, _both() | B.R_CSR | B.R_STATUS, NO_RUNE_OFFSETS | OFFSETS_ONLY, pairs=(1,),
                   om=oracle_models(MODELS_DE[0]))
    assert len(r.tok_rblk) == 0 and len(r.tok_bblk) == 23000 + 90
    r, _, _ = _run(gpu(MODELS_DE[0]), docs, _both() | B.R_CSR | B.R_STATUS, NO_BYTE_OFFSETS | OFFSETS_ONLY, pairs=(0,),
                   om=oracle_models(MODELS_DE[0]))
    assert len(r.tok_bblk) == 0 and len(r.tok_rblk) == 23000 + 90


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["datok", "matok"])
def test_blocks_are_packed_after_the_exact_pass(tmp_path, kind):
    """Crafted documents whose rows the exact pass rewrites (calls out of position order): the blocked form holds the
    rewritten rows."""
    import gzip
    import datok_amd
    from oracle import oracle as O
    B = _B()
    blob = getattr(craft, kind)(kind == "matok")     # (the matrix needs the triple sentence end to get there)
    path = tmp_path / ("crafted." + kind)
    path.write_bytes(blob)
    tok, om = datok_amd.load_tokenizer_file(str(path)), O.Model(raw=gzip.decompress(blob))
    docs = [b"ab ab. " * 30, b"ab ab. " * 3 + b"a\x04a b. " * 20, b"a. b. " * 20 + b"a\x04a ab.", b"ab\x04ab a\x04b. a " * 25]
    in_contract = [d for d, doc in enumerate(docs) if om.transduce_doc(doc, 0).status == 0]
    assert len(in_contract) >= 3          # (the last one has a text without a token: only its status is compared)
    from datok_amd import corpus
    text, off = corpus.concat_docs(docs)
    with B(len(text), len(docs)) as b:
        b.set_input(text, off)
        b.run(tok, 0)
        r, _ = _blocked_result(b, _both() | B.R_CSR | B.R_STATUS)
        assert any(d in r.exact for d in in_contract) and b.totals()["n_tokens"] > 128
        assert assert_batch_equals_oracle(om, r, text, off, fields=[f for p in PAIRS for f in p]) == len(in_contract)


@pytest.mark.gpu
def test_pipeline_with_ragged_slices(gpu, oracle_models):
    """Slices of 256 KiB, depth 2, one document of 100 KB among short ones: every document decoded in the callback
    equals the oracle."""
    import datok_amd
    from datok_amd import corpus
    B = _B()
    tok, om = gpu(MODELS_DE[0]), oracle_models(MODELS_DE[0])
    t, o = corpus.german_docs(60, 9000, seed=29)
    docs = [t[int(o[d]):int(o[d + 1])].tobytes()[:1500 + 125 * d].rsplit(b" ", 1)[0] for d in range(60)]
    docs.insert(31, blocked.five_documents()[0])
    text, off = corpus.concat_docs(docs)
    seen = []

    def on_slice(first, n, b):
        r = b.result(copy=False)
        nt = b.totals()["n_tokens"]
        assert len(r.tok_rblk) == nt and len(r.tok_rblk_head) == (nt + 63) // 64 and len(r.tok_rstart) == 0 and len(r.tok_bblk) == 0
        sub = (off[first:first + n + 1] - off[first]).astype(np.uint64)
        assert assert_batch_equals_oracle(om, r, text[int(off[first]):int(off[first + n])], sub,
                                          fields=("tok_rstart", "tok_rend")) == n
        seen.append(n)
    with datok_amd.Pipeline(256 << 10, 64, depth=2) as p:
        p.set_result_fields(B.R_TOK_RUNE_BLK | B.R_CSR | B.R_STATUS)
        p.run(tok, text, off, 0, on_slice)
    assert sum(seen) == len(docs) and len(seen) >= 2
