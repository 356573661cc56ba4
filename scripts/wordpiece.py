#!/usr/bin/env python3
"""What splitting every token into WordPiece ids costs (dtk_batch_set_wordpiece), on the bench
batch: 4096 x 4 KiB German documents on tokenizer_de.matok.

The generated corpus has only a few thousand distinct surfaces and a few hundred of them make up nearly all of its
tokens, so the vocabulary does not hold them all: the most frequent surfaces until they cover COVER of the tokens, every
single character of the others as a first piece and as a ## piece, and ## pieces of two to four characters cut from the
others.  The share of tokens that splits is printed.  The kernels are timed a second time over a vocabulary built the
same way whose whole surfaces cover COVER_WORDS of the tokens: nearly every token a word, what the whole-remainder-first
search order is made for.

  kernel     per fresh run, on the batch's download stream between HIP events: first the lookup of dtk_batch_set_vocab
             as dtk_batch_download_begin enqueues it (k_token_ids), then -- the split attached afterwards -- the three
             launches of dtk_wordpiece.hip with the clear and the copy of their counters; median of the samples behind a
             warm-up.  Beside them the same batch's walk stage.
  pipeline   host text in -> host results out through dtk_pipeline_run from page-locked text, 24 slices, depth 4,
             the legs alternated:
             leg pieces   piece_off, piece_id and piece_bend come home with R_CSR | R_STATUS
             leg ids      the ids of dtk_pipeline_set_vocab come home (4 B per token)
             leg offsets  the route without the feature, first half: R_TOK_BYTE | R_CSR home (8 B per token)
  host       ... second half: every surface of ONE slice sliced out of the text and split on one core in this
             interpreter, without and with a cache per distinct surface (the generated corpus flatters the cache), and
             with the tokenizers package's compiled WordPiece where it is installed

Nothing is gated.  Everything runs in one child process without torch.

usage: python scripts/wordpiece.py [--reps 5] [--out profiles/wordpiece.txt]
"""
import argparse
import collections
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODEL = os.path.join(ROOT, "tests", "golden", "models", "tokenizer_de.matok")
OFFSETS_ONLY, NO_RUNE_OFFSETS = 256, 1024
FLAGS = OFFSETS_ONLY | NO_RUNE_OFFSETS
N_DOCS, DOC_BYTES, COVER, COVER_WORDS = 4096, 4096, 0.75, 0.999
SLICES, DEPTH = 24, 4
PREFIX = b"##"


def surfaces_of(raw, off, r):
    out = []
    for d in range(len(off) - 1):
        base = int(off[d])
        for i in range(int(r.tok_off[d]), int(r.tok_off[d + 1])):
            out.append(raw[base + int(r.tok_bstart[i]):base + int(r.tok_bend[i])])
    return out


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def build_vocabulary(freq, cover=COVER):
    """[UNK], the most frequent surfaces whole, and for the others their characters and chunks of them."""
    ranked = [w for w, _ in freq.most_common()]
    n_whole, covered, total = 0, 0, sum(freq.values())
    while covered < cover * total:
        covered += freq[ranked[n_whole]]
        n_whole += 1
    whole, rest = ranked[:n_whole], ranked[n_whole:]
    firsts, conts = set(), set()
    for k, s in enumerate(rest):
        chars = [c.encode() for c in s.decode("utf-8")]
        if k % 7 == 6:
            continue                                # (a seventh of them gets nothing: some tokens stay unknown)
        firsts.add(chars[0])
        firsts.add(b"".join(chars[:3]))
        conts.update(PREFIX + c for c in chars[1:])
        for n in (2, 3, 4):
            conts.update(PREFIX + b"".join(chars[i:i + n]) for i in range(3, len(chars), n))
    words = [b"[UNK]"] + whole + sorted(firsts - set(whole)) + sorted(conts)
    return words, n_whole


def host_split(table, key, unk_id=0, max_runes=100):
    """BERT's WordPiece over bytes, cuts on rune boundaries: [(id, end)]."""
    ends = [e for e in range(1, len(key) + 1) if e == len(key) or (key[e] & 0xC0) != 0x80]
    if len(ends) > max_runes:
        return [(unk_id, len(key))]
    out, start = [], 0
    while start < len(key):
        for end in reversed(ends):
            if end <= start:
                return [(unk_id, len(key))]
            w = key[start:end] if start == 0 else PREFIX + key[start:end]
            i = table.get(w)
            if i is not None:
                out.append((i, end))
                start = end
                break
        else:
            return [(unk_id, len(key))]
    return out


def kernel_times(tok, text, off, vocab, say, label, samples=20):
    import datok_amd
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    ev = [C.c_void_p() for _ in range(4)]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)))
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_profiling(True)
        b.set_result_fields(0)                      # the download is the lookup, then the split, alone
        b.set_input(text, off)
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        b.set_vocab(vocab, ids_home=False)
        ids_us, wp_us = [], []
        for k in range(samples + 3):                # (the first three are the warm-up)
            b.set_wordpiece(None)
            b.run(tok, FLAGS)
            tot = b.totals()                        # the run is complete: what follows is the lookup alone
            ok(hip.hipEventRecord(ev[0], stream))
            b.download_begin()
            ok(hip.hipEventRecord(ev[1], stream))
            b.set_wordpiece(vocab, prefix=PREFIX, pieces_home=False)
            ok(hip.hipEventRecord(ev[2], stream))
            b.download_begin()                      # (the ids are there: this enqueues the split alone)
            ok(hip.hipEventRecord(ev[3], stream))
            ok(hip.hipEventSynchronize(ev[3]))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
            a = ms.value * 1e3
            ok(hip.hipEventElapsedTime(C.byref(ms), ev[2], ev[3]))
            if k >= 3:
                ids_us.append(a)
                wp_us.append(ms.value * 1e3)
        stages = b.stage_ms()
        v = b.pieces(device=True)
        say(json.dumps({"vocabulary_covers": label, "split_us_median": round(median(wp_us), 1), "split_us_min": round(min(wp_us), 1),
                        "split_us_max": round(max(wp_us), 1), "k_token_ids_us_median": round(median(ids_us), 1),
                        "k_token_ids_us_min": round(min(ids_us), 1), "k_token_ids_us_max": round(max(ids_us), 1),
                        "samples": len(wp_us), "tokens": tot["n_tokens"], "pieces": int(v.n_pieces),
                        "unknown_tokens": int(v.n_unknown), "bytes": int(off[-1]),
                        "Gtok_per_s": round(tot["n_tokens"] / median(wp_us) / 1e3, 2),
                        "walk_us": round(stages["walk"] * 1e3, 1), "all_stages_us": round(sum(stages.values()) * 1e3, 1)}))
    for e in ev:
        ok(hip.hipEventDestroy(e))


def pipeline_rates(tok, inputs, vocab, reps, say):
    import datok_amd
    B = datok_amd.Batch
    total = int(inputs[0][1][-1])
    pin = datok_amd.PinnedBuffer(total * SLICES)
    for i in range(SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(SLICES)])
    seen = {"tokens": 0, "pieces": 0, "sum": 0}

    def cb_pieces(first, n, bb):
        p = bb.pieces(copy=False)                   # (came home with the slice: this waits, and fetches what the first copies left out)
        seen["tokens"] += len(p.piece_off) - 1
        seen["pieces"] += p.n_pieces
        seen["sum"] += int(p.piece_id[-1]) + int(p.piece_bend[-1])

    def cb_ids(first, n, bb):
        ids, unknown = bb.token_ids(copy=False)
        seen["tokens"] += len(ids)
        seen["sum"] += int(ids[-1]) + unknown

    def cb_offsets(first, n, bb):
        res = bb.result(copy=False)
        seen["tokens"] += len(res.tok_bend)
        seen["sum"] += int(res.tok_bend[-1])
    legs = {}
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_wordpiece(vocab, prefix=PREFIX, pieces_home=True)
    p.set_result_fields(B.R_CSR | B.R_STATUS)
    legs["pieces"] = (p, cb_pieces)
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_vocab(vocab, ids_home=True)
    p.set_result_fields(B.R_CSR | B.R_STATUS)
    legs["ids"] = (p, cb_ids)
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_result_fields(B.R_TOK_BYTE | B.R_CSR)
    legs["offsets"] = (p, cb_offsets)
    for p, cb in legs.values():
        p.run(tok, pin.array, big_off, FLAGS, cb)   # allocations, lane plans, page-locked buffers
    rates = {leg: [] for leg in legs}
    n_tok = n_pieces = 0
    for rep in range(reps):
        for leg, (p, cb) in legs.items():           # the legs alternate
            seen.update(tokens=0, pieces=0, sum=0)
            t0 = time.perf_counter()
            p.run(tok, pin.array, big_off, FLAGS, cb)
            rates[leg].append(total * SLICES / (time.perf_counter() - t0) / 1e9)
            n_tok = seen["tokens"]
            n_pieces = max(n_pieces, seen["pieces"])
    for leg, v in rates.items():
        say(json.dumps({"pipeline_leg": leg, "GBps_median": round(median(v), 2), "GBps_min": round(min(v), 2),
                        "GBps_max": round(max(v), 2), "runs": len(v), "slices": SLICES, "depth": DEPTH,
                        "slice_bytes": total, "tokens": n_tok, "pieces": n_pieces if leg == "pieces" else None}))
    for p, _ in legs.values():
        p.close()
    pin.close()
    return {leg: median(v) for leg, v in rates.items()}


def child(args):
    import datok_amd
    from datok_amd import corpus
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    datok_amd.lib().dtk_set_device(0)
    tok = datok_amd.load_tokenizer_file(MODEL)
    assert tok is not None
    inputs = [corpus.german_docs(N_DOCS, DOC_BYTES, seed=2 + k) for k in range(3)]
    text, off = inputs[0]
    raw = bytes(text)
    B = datok_amd.Batch
    with B(len(text), N_DOCS) as b:                 # the corpus' surfaces, for the vocabulary
        b.set_input(text, off)
        b.set_result_fields(B.R_TOK_BYTE | B.R_CSR)
        b.run(tok, FLAGS)
        r = b.result()
    surf = surfaces_of(raw, off, r)
    freq = collections.Counter(surf)
    words, n_whole = build_vocabulary(freq)
    table = {}
    for i, w in enumerate(words):
        table.setdefault(w, i)
    vocab = datok_amd.Vocab(words)
    # the route without the feature, second half: one core, one slice, this interpreter
    t0 = time.perf_counter()
    host = [host_split(table, s) for s in surfaces_of(raw, off, r)]
    host_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    memo = {}
    for s in surfaces_of(raw, off, r):
        if s not in memo:
            memo[s] = host_split(table, s)
    cached_s = time.perf_counter() - t0
    n_split = sum(1 for h in host if len(h) > 1)
    n_unknown = sum(1 for s, h in zip(surf, host) if h == [(0, len(s))] and s != b"[UNK]")
    say(json.dumps({"vocabulary_covers": COVER, "library": os.path.relpath(datok_amd._lib.LIB_PATH, ROOT), "docs": N_DOCS, "doc_bytes": DOC_BYTES,
                    "tokens": len(surf), "distinct_surfaces": len(freq), "vocabulary": len(words), "whole_surfaces": n_whole,
                    "vocabulary_bytes": sum(map(len, words)), "longest_word": max(map(len, words)),
                    "tokens_split_share": round(n_split / len(surf), 4), "tokens_unknown_share": round(n_unknown / len(surf), 4),
                    "pieces_per_token": round(sum(map(len, host)) / len(surf), 3)}))
    with B(len(text), N_DOCS) as b:                 # (and the device's pieces are these)
        b.set_input(text, off)
        b.set_wordpiece(vocab, prefix=PREFIX)
        b.run(tok, FLAGS)
        got = b.pieces()
        rr = b.result()
    flat = [x for h in host for x in h]
    d_of = np.repeat(np.arange(N_DOCS), np.diff(rr.tok_off.astype(np.int64)))
    t_of = np.repeat(np.arange(len(surf)), np.diff(got.piece_off.astype(np.int64)))
    assert np.array_equal(np.diff(got.piece_off.astype(np.int64)), np.array([len(h) for h in host]))
    assert np.array_equal(got.piece_id, np.array([i for i, _ in flat], np.int32))
    assert np.array_equal(got.piece_bend.astype(np.int64), rr.tok_bstart[t_of].astype(np.int64) + np.array([e for _, e in flat]))
    assert got.n_unknown == n_unknown and len(d_of) == len(surf)
    kernel_times(tok, text, off, vocab, say, COVER)
    # nearly every token a word: the other end of the divergence
    words2, n_whole2 = build_vocabulary(freq, COVER_WORDS)
    table2 = {}
    for i, w in enumerate(words2):
        table2.setdefault(w, i)
    split2 = {s: host_split(table2, s) for s in freq}
    say(json.dumps({"vocabulary_covers": COVER_WORDS, "vocabulary": len(words2), "whole_surfaces": n_whole2,
                    "tokens_split_share": round(sum(n for s, n in freq.items() if len(split2[s]) > 1) / len(surf), 4),
                    "tokens_unknown_share": round(sum(n for s, n in freq.items() if split2[s] == [(0, len(s))] and s != b"[UNK]") / len(surf), 4),
                    "pieces_per_token": round(sum(n * len(split2[s]) for s, n in freq.items()) / len(surf), 3)}))
    kernel_times(tok, text, off, datok_amd.Vocab(words2), say, COVER_WORDS)
    med = pipeline_rates(tok, inputs, vocab, args.reps, say)
    rate = len(text) / host_s / 1e9
    say(json.dumps({"host_split_one_slice_s": round(host_s, 2), "host_split_GBps": round(rate, 4),
                    "with_a_cache_per_surface_s": round(cached_s, 2), "with_a_cache_GBps": round(len(text) / cached_s / 1e9, 4),
                    "tokens": len(surf),
                    "what": "slicing every surface out of the text and a WordPiece over a dict, one core, CPython; "
                            "pieces equal the device's"}))
    try:
        import tokenizers
        model = tokenizers.models.WordPiece(vocab={w.decode("utf-8"): i for w, i in table.items() if _utf8(w)},
                                            unk_token="[UNK]", continuing_subword_prefix="##")
        strs = [s.decode("utf-8") for s in surf]
        t0 = time.perf_counter()
        n = sum(len(model.tokenize(s)) for s in strs)
        tk_s = time.perf_counter() - t0
        say(json.dumps({"tokenizers_wordpiece_one_slice_s": round(tk_s, 2), "tokenizers_GBps": round(len(text) / tk_s / 1e9, 4),
                        "pieces": n, "what": "tokenizers.models.WordPiece.tokenize per surface (surfaces already cut and decoded)"}))
    except ImportError:
        say(json.dumps({"tokenizers": "not installed"}))
    both = 1 / (1 / med["offsets"] + 1 / rate)
    say("medians GB/s of input: pieces home %.2f, ids home %.2f; without the feature: offsets home %.2f, then the host "
        "split at %.4f -- one after the other %.4f" % (med["pieces"], med["ids"], med["offsets"], rate, both))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def _utf8(w):
    try:
        w.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the raw lines and the summary to this file")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    cmd += ["--out", args.out] if args.out else []
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_") or k == "DATOK_GPU_LIB"}
    return subprocess.run(cmd, env=env, timeout=900).returncode


if __name__ == "__main__":
    sys.exit(main())
