#!/usr/bin/env python3
"""What looking every token up in a vocabulary costs (dtk_batch_set_vocab), on the bench batch:
4096 x 4 KiB German documents on tokenizer_de.matok, the vocabulary the 50 000 most frequent surfaces of that corpus.

  kernel     the lookup as dtk_batch_download_begin enqueues it -- the clear of the unknown counter, k_token_ids, the
             copy of the counter -- between two HIP events on the batch's download stream, with and without a tally;
             a fresh run per sample (the lookup runs once per run), median of the samples behind a warm-up.  Beside it
             the same batch's symbolise, walk and compaction stages (dtk_batch_stage_ms).
  pipeline   host text in -> host results out through dtk_pipeline_run from page-locked text, 24 slices, depth 4:
             leg ids      the ids come home (4 B per token) with R_CSR | R_STATUS
             leg counts   a tally alone: nothing per token leaves the device
             leg offsets  the route without the feature, first half: R_TOK_BYTE | R_CSR home (8 B per token)
  host       ... second half: every surface of ONE slice sliced out of the text and looked up in a dict on one core,
             in this interpreter (a compiled loop would be faster; the figure says what this script's caller pays)

Nothing is gated.  Everything runs in one child process without torch.

usage: python scripts/token_ids.py [--reps 5] [--out profiles/token_ids.txt]
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
N_DOCS, DOC_BYTES, N_WORDS = 4096, 4096, 50000
SLICES, DEPTH = 24, 4


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


def kernel_times(tok, text, off, vocab, say, samples=20):
    import datok_amd
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    tally = datok_amd.Tally(vocab)
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_profiling(True)
        b.set_result_fields(0)                      # the download is the lookup alone
        b.set_input(text, off)
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        for name, t in (("without a tally", None), ("with a tally", tally)):
            b.set_vocab(vocab, tally=t, ids_home=False)
            us = []
            for k in range(samples + 3):            # (the first three are the warm-up)
                b.run(tok, FLAGS)
                tot = b.totals()                    # the run is complete: what follows is the lookup alone
                ok(hip.hipEventRecord(e0, stream))
                b.download_begin()
                ok(hip.hipEventRecord(e1, stream))
                ok(hip.hipEventSynchronize(e1))
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
                if k >= 3:
                    us.append(ms.value * 1e3)
            stages = b.stage_ms()
            v = b.token_ids(device=True)
            say(json.dumps({"lookup": name, "us_median": round(median(us), 1), "us_min": round(min(us), 1),
                            "us_max": round(max(us), 1), "samples": len(us), "tokens": tot["n_tokens"],
                            "unknown": int(v.n_unknown), "bytes": int(off[-1]),
                            "Gtok_per_s": round(tot["n_tokens"] / median(us) / 1e3, 2),
                            "symbolise_us": round(stages["symbolize"] * 1e3, 1), "walk_us": round(stages["walk"] * 1e3, 1),
                            "compaction_us": round(stages["compact"] * 1e3, 1),
                            "all_stages_us": round(sum(stages.values()) * 1e3, 1)}))
        counts = tally.read()
        assert int(counts.sum()) == (samples + 3) * tot["n_tokens"]
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))


def pipeline_rates(tok, inputs, vocab, reps, say):
    import datok_amd
    B = datok_amd.Batch
    total = int(inputs[0][1][-1])
    pin = datok_amd.PinnedBuffer(total * SLICES)
    for i in range(SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(SLICES)])
    tally = datok_amd.Tally(vocab)
    seen = {"tokens": 0, "sum": 0}

    def cb_ids(first, n, bb):
        ids, unknown = bb.token_ids(copy=False)     # (came home with the slice: this only waits)
        seen["tokens"] += len(ids)
        seen["sum"] += int(ids[-1]) + unknown

    def cb_offsets(first, n, bb):
        res = bb.result(copy=False)
        seen["tokens"] += len(res.tok_bend)
        seen["sum"] += int(res.tok_bend[-1])
    legs = {}
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_vocab(vocab, ids_home=True)
    p.set_result_fields(B.R_CSR | B.R_STATUS)
    legs["ids"] = (p, cb_ids)
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_vocab(vocab, tally=tally, ids_home=False)
    legs["counts"] = (p, None)
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_result_fields(B.R_TOK_BYTE | B.R_CSR)
    legs["offsets"] = (p, cb_offsets)
    for p, cb in legs.values():
        p.run(tok, pin.array, big_off, FLAGS, cb)   # allocations, lane plans, page-locked buffers
    rates = {leg: [] for leg in legs}
    for rep in range(reps):
        for leg, (p, cb) in legs.items():           # the legs alternate
            seen.update(tokens=0, sum=0)
            t0 = time.perf_counter()
            p.run(tok, pin.array, big_off, FLAGS, cb)
            rates[leg].append(total * SLICES / (time.perf_counter() - t0) / 1e9)
            if leg != "counts":
                n_tok = seen["tokens"]
    down = {"ids": 4, "counts": 0, "offsets": 8}
    for leg, v in rates.items():
        say(json.dumps({"pipeline_leg": leg, "GBps_median": round(median(v), 2), "GBps_min": round(min(v), 2),
                        "GBps_max": round(max(v), 2), "runs": len(v), "slices": SLICES, "depth": DEPTH,
                        "slice_bytes": total, "down_B_per_token": down[leg], "tokens": n_tok}))
    counts = tally.read()
    assert int(counts.sum()) == (reps + 1) * n_tok
    say(json.dumps({"tally_tokens_per_run": n_tok, "unknown_share": round(float(counts[-1]) / float(counts.sum()), 4)}))
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
    words = [w for w, _ in freq.most_common(N_WORDS)]
    vocab = datok_amd.Vocab(words)
    say(json.dumps({"library": os.path.relpath(datok_amd._lib.LIB_PATH, ROOT), "docs": N_DOCS, "doc_bytes": DOC_BYTES,
                    "tokens": len(surf), "distinct_surfaces": len(freq), "vocabulary": len(words),
                    "vocabulary_bytes": sum(map(len, words))}))
    kernel_times(tok, text, off, vocab, say)
    med = pipeline_rates(tok, inputs, vocab, args.reps, say)
    # the route without the feature, second half: one core, one slice, this interpreter
    table = {w: i for i, w in enumerate(words)}
    t0 = time.perf_counter()
    ids = np.fromiter((table.get(s, -1) for s in surfaces_of(raw, off, r)), dtype=np.int32, count=len(surf))
    host_s = time.perf_counter() - t0
    with B(len(text), N_DOCS) as b:                 # (and the device's ids are these)
        b.set_input(text, off)
        b.set_vocab(vocab)
        b.run(tok, FLAGS)
        got, unknown = b.token_ids()
    assert np.array_equal(got, ids) and unknown == int((ids < 0).sum())
    host = len(text) / host_s / 1e9
    say(json.dumps({"host_lookup_one_slice_s": round(host_s, 2), "host_lookup_GBps": round(host, 4), "tokens": len(surf),
                    "what": "slicing every surface out of the text and a dict lookup, one core, CPython; ids equal the device's"}))
    both = 1 / (1 / med["offsets"] + 1 / host)
    say("medians GB/s of input: ids home %.2f, counts only %.2f; without the feature: offsets home %.2f, then the host "
        "lookup at %.4f -- one after the other %.4f" % (med["ids"], med["counts"], med["offsets"], host, both))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


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
