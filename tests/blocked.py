"""The blocked form of a pair of token offset arrays (DTK_R_TOK_RUNE_BLK / DTK_R_TOK_BYTE_BLK), in plain numpy
(test infrastructure).

Written from the format's description in include/datok_gpu.h, not from the kernel: it is the CPU-side definition
that the decoders (datok_amd.unpack_blocked, dtk_blk_start / dtk_blk_end) and k_pack_blk are compared against.

Tokens are taken in the batch-wide order of the result arrays; block j holds the tokens [64j, 64j + 64).
    brk   = the smallest lane l >= 1 of the block with start[64j + l] < end[64j + l - 1], or 64 if there is none
    base0 = the minimum over every start and end of the lanes < brk
    base1 = the minimum over the lanes >= brk, or 0 if brk == 64
    word  = (start - base) | (end - base) << 16      with base = lane < brk ? base0 : base1
A block overflows if in either segment maximum - minimum exceeds the span limit (65 535).
"""
import numpy as np

BLOCK = 64
SPAN = 65535


def encode(start, end, span=SPAN):
    """(words uint32[n], heads int32[ceil(n / 64), 4] = base0, base1, brk, reserved, overflowing blocks, worst span)."""
    start, end = np.asarray(start).astype(np.int64), np.asarray(end).astype(np.int64)
    assert start.shape == end.shape and start.ndim == 1
    n = len(start)
    words = np.zeros(n, dtype=np.uint32)
    heads = np.zeros(((n + BLOCK - 1) // BLOCK, 4), dtype=np.int32)
    overflow = worst = 0
    for j in range(len(heads)):
        s, e = start[BLOCK * j:BLOCK * j + BLOCK], end[BLOCK * j:BLOCK * j + BLOCK]
        dec = np.flatnonzero(s[1:] < e[:-1])
        brk = int(dec[0]) + 1 if len(dec) else BLOCK
        both = np.concatenate([s[:brk], e[:brk]])
        base0, span0 = int(both.min()), int(both.max() - both.min())
        base1 = span1 = 0
        if brk < BLOCK:
            both = np.concatenate([s[brk:], e[brk:]])
            base1, span1 = int(both.min()), int(both.max() - both.min())
        base = np.where(np.arange(len(s)) < brk, base0, base1)
        words[BLOCK * j:BLOCK * j + len(s)] = ((s - base) & 0xFFFF) | (((e - base) & 0xFFFF) << 16)
        heads[j] = (base0, base1, brk, 0)
        overflow += int(max(span0, span1) > span)
        worst = max(worst, span0, span1)
    return words, heads, overflow, worst


# ---- the batch the format was checked on: long running text, a tiny document, long text again, one document of three
#      EOT-separated texts, and tokens of 1000 bytes each
def five_documents():
    from datok_amd import corpus
    t, _ = corpus.german_docs(4, 100000, seed=41)
    run = [t[k * 100000:(k + 1) * 100000].tobytes() for k in range(4)]
    def cut(doc, a, z):   # (on blanks: no rune is cut)
        return doc[a:z].split(b" ", 1)[1].rsplit(b" ", 1)[0]
    texts = cut(run[2], 0, 68400) + b"\n\x04\n" + cut(run[3], 0, 68400) + b"\n\x04\n" + cut(run[2], 30000, 98400) + b"\n"
    long_tokens = b"".join(bytes([97 + k % 26]) * 1000 + b" " for k in range(71))
    return [run[0], b"Ein Baum.", run[1], texts, long_tokens]


_oracle_cache = {}


def oracle_batch(om, key, docs, flags=0):
    """The oracle's token arrays of `docs` in batch order: dict of tok_off, status and the four offset arrays.
    Computed once per `key` and shared (read only)."""
    if key not in _oracle_cache:
        rows = [om.transduce_doc(d, flags) for d in docs]
        out = {f: np.concatenate([getattr(r, f) for r in rows]) for f in ("tok_rstart", "tok_rend", "tok_bstart", "tok_bend")}
        out["tok_off"] = np.concatenate([[0], np.cumsum([len(r.tok_rstart) for r in rows])]).astype(np.uint64)
        out["status"] = np.array([r.status for r in rows], dtype=np.uint32)
        for a in out.values():
            a.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]
