#!/usr/bin/env python3
"""What the 16-bit blocked token offsets (DTK_R_TOK_RUNE_BLK) buy on the way home: host text in
-> host rune offsets out through dtk_pipeline_run, from page-locked text, 24 slices of 16 MiB, depth 4 -- the 32-bit
arrays, the int16 pairs where they exist, and the blocks, on the same machine in the same run.

  corpus a  256 x 64 KiB German documents per slice (longer than 32 767 bytes: no int16 pairs)   32-bit | blocked
  corpus b  the bench's 4096 x 4 KiB documents per slice                                         32-bit | int16 | blocked

and the time of k_pack_blk against k_pack_r16 on the token arrays of one slice of corpus b, with HIP events on the
batch's download stream (both launchers called directly on the arrays of dtk_batch_result_device).

Everything runs in one child process without torch.  The forms are alternated and repeated; per form the GB/s of every
timed run (median, min .. max).  Nothing is gated: the summary says whether the blocked form beat the 32-bit one.

usage: python scripts/blocked_offsets.py [--reps 3] [--out profiles/blocked_offsets.txt]
"""
import argparse
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
RUN_FLAGS = 256 | 512     # bench.py's: offsets only, rune offsets
SLICES, DEPTH = 24, 4
CORPORA = {"a": (256, 65536, ("wide", "blk")), "b": (4096, 4096, ("wide", "r16", "blk"))}


def forms():
    import datok_amd
    B = datok_amd.Batch
    rest = B.R_SENT | B.R_CSR | B.R_STATUS
    return {"wide": B.R_TOK_RUNE | rest, "r16": B.R_TOK_RUNE16 | rest, "blk": B.R_TOK_RUNE_BLK | rest}


def pipeline_rates(tok, name, reps, say):
    import datok_amd
    from datok_amd import corpus
    n_docs, doc_bytes, which = CORPORA[name]
    inputs = [corpus.german_docs(n_docs, doc_bytes, seed=2 + k) for k in range(3)]
    total = int(inputs[0][1][-1])
    pin = datok_amd.PinnedBuffer(total * SLICES)
    for i in range(SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(SLICES)])
    fields = forms()
    seen = {"tokens": 0, "bytes": 0, "sum": 0}

    def on_slice(form):
        def cb(first, n, bb):
            t = bb.totals()
            res = bb.result(copy=False)       # host pointers into the slice's page-locked buffers
            got = {"wide": res.tok_rend, "r16": res.tok_r16, "blk": res.tok_rblk}[form]
            assert len(got) == t["n_tokens"], (form, len(got), t["n_tokens"])   # (the form asked for, not a stand-in)
            seen["tokens"] += t["n_tokens"]
            seen["bytes"] += (8 if form == "wide" else 4) * t["n_tokens"] + 4 * t["n_sent"] + 28 * n + \
                (16 * len(res.tok_rblk_head) if form == "blk" else 0)
            seen["sum"] += int(got.reshape(-1)[-1]) + int(res.tok_off[-1])
        return cb
    pipes = {}
    for form in which:
        pipes[form] = datok_amd.Pipeline(total, n_docs, depth=DEPTH)
        pipes[form].set_result_fields(fields[form])
        pipes[form].run(tok, pin.array, big_off, RUN_FLAGS, on_slice(form))   # allocations, lane plans, page-locked buffers
    rates = {form: [] for form in which}
    per_byte = {}
    for rep in range(reps):
        for form in which:
            seen.update(tokens=0, bytes=0)
            t0 = time.perf_counter()
            pipes[form].run(tok, pin.array, big_off, RUN_FLAGS, on_slice(form))
            rates[form].append(total * SLICES / (time.perf_counter() - t0) / 1e9)
            per_byte[form] = seen["bytes"] / (total * SLICES)
    for p in pipes.values():
        p.close()
    pin.close()
    for form in which:
        v = sorted(rates[form])
        say(json.dumps({"corpus": name, "docs_per_slice": n_docs, "doc_bytes": doc_bytes, "form": form,
                        "down_B_per_input_byte": round(per_byte[form], 3), "GBps_median": round(v[len(v) // 2], 2),
                        "GBps_min": round(v[0], 2), "GBps_max": round(v[-1], 2), "runs": len(v)}))
    return {form: sorted(v)[len(v) // 2] for form, v in rates.items()}, inputs[0]


class _Pair(C.Structure):
    _fields_ = [("start", C.c_void_p), ("end", C.c_void_p), ("words", C.c_void_p), ("heads", C.c_void_p), ("flag", C.c_void_p)]


class _PackArgs(C.Structure):   # DtkPackBlkArgs, dtk_internal.h
    _fields_ = [("pair", _Pair * 2), ("n_pairs", C.c_uint32), ("span", C.c_uint32), ("n", C.c_uint64)]


def kernel_times(tok, text, off, say, launches=20):
    """k_pack_r16 and k_pack_blk (one pair) on the rune offsets of one slice, microseconds per launch."""
    import datok_amd
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_input(text, off)
        b.run(tok, RUN_FLAGS)
        n = b.totals()["n_tokens"]
        v = b.result_device()
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        words, heads, flag = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ok(hip.hipMalloc(C.byref(words), C.c_size_t(4 * n)))
        ok(hip.hipMalloc(C.byref(heads), C.c_size_t(16 * ((n + 63) // 64))))
        ok(hip.hipMalloc(C.byref(flag), C.c_size_t(4)))
        ok(hip.hipMemset(flag, 0, C.c_size_t(4)))
        a = _PackArgs()
        a.pair[0] = _Pair(v.tok_rstart, v.tok_rend, words, heads, flag)
        a.n_pairs, a.span, a.n = 1, 65535, n
        L.dtk_launch_pack_blk.argtypes = [C.POINTER(_PackArgs), C.c_void_p]
        L.dtk_launch_pack_r16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        kernels = {"k_pack_r16": lambda: L.dtk_launch_pack_r16(v.tok_rstart, v.tok_rend, words, n, stream),
                   "k_pack_blk": lambda: L.dtk_launch_pack_blk(C.byref(a), stream)}
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        us = {k: [] for k in kernels}
        for rep in range(4):                      # (the first round is the warm-up)
            for name, launch in kernels.items():
                ok(hip.hipEventRecord(e0, stream))
                for _ in range(launches):
                    ok(launch())
                ok(hip.hipEventRecord(e1, stream))
                ok(hip.hipEventSynchronize(e1))
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
                if rep:
                    us[name].append(ms.value * 1e3 / launches)
        for p in (words, heads, flag):
            ok(hip.hipFree(p))
        ok(hip.hipEventDestroy(e0))
        ok(hip.hipEventDestroy(e1))
    out = {k: round(sorted(x)[len(x) // 2], 2) for k, x in us.items()}
    say(json.dumps({"kernel_us_per_launch": out, "tokens": n, "launches_per_sample": launches,
                    "blk_over_r16": round(out["k_pack_blk"] / out["k_pack_r16"], 2),
                    "what": "back to back on the download stream, between two HIP events; 8 B read per token, "
                            "4 resp. 4.25 B written"}))
    return out


def child(args):
    import datok_amd
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    datok_amd.lib().dtk_set_device(0)
    tok = datok_amd.load_tokenizer_file(MODEL)
    assert tok is not None
    ra, _ = pipeline_rates(tok, "a", args.reps, say)
    rb, one = pipeline_rates(tok, "b", args.reps, say)
    kernel_times(tok, one[0], one[1], say)
    say("corpus a: blocked / 32-bit = %.3f  (blocked beats the 32-bit form: %s)" % (ra["blk"] / ra["wide"], "yes" if ra["blk"] > ra["wide"] else "NO"))
    say("corpus b: blocked / 32-bit = %.3f  (not slower: %s);  blocked / int16 pairs = %.3f"
        % (rb["blk"] / rb["wide"], "yes" if rb["blk"] >= rb["wide"] else "NO", rb["blk"] / rb["r16"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the raw lines and the summary to this file")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)] + (["--out", args.out] if args.out else [])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_") or k == "DATOK_GPU_LIB"}
    return subprocess.run(cmd, env=env, timeout=900).returncode


if __name__ == "__main__":
    sys.exit(main())
