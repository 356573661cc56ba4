#!/usr/bin/env python3
"""What the event list (DTK_R_EVENT_LIST) buys a closure replay on the way home: host text in ->
everything a custom TokenWriter's replay reads out, through dtk_pipeline_run from page-locked text, 24 slices of
16 MiB, depth 4, on the same machine in the same run:

  leg a  R_EVENTS     | R_TOK_BYTE_BLK | R_CSR | R_STATUS    the five event bitmaps (the narrowest download before the list)
  leg b  R_EVENT_LIST | R_TOK_BYTE_BLK | R_CSR | R_STATUS    the list

  corpus 4k   the bench's 4096 x 4 KiB German documents per slice
  corpus 64k  256 x 64 KiB documents per slice

and the time of the list's four kernels on the bitmaps of one slice of corpus 4k, with HIP events on the batch's
download stream (the launcher called directly, 20 launches back to back).

Everything runs in one child process without torch.  The legs are alternated and repeated; per leg the GB/s of every
timed run (median, min .. max), the bytes downloaded per input byte and the list's entries against the bound
n_sent + n_texts.  Nothing is gated: the summary says whether the slowest run of b beat the fastest run of a.

--legs a runs on a build without the field too (DATOK_GPU_LIB selects the library): the comparison with the parent.

usage: python scripts/event_list.py [--reps 3] [--legs ab] [--out profiles/event_list.txt]
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
RUN_FLAGS = 256 | 1024    # offsets only, byte offsets: what a closure replay reads
SLICES, DEPTH = 24, 4
CORPORA = {"4k": (4096, 4096), "64k": (256, 65536)}
R_EVENT_LIST = 2048


def fields(leg):
    import datok_amd
    B = datok_amd.Batch
    return (B.R_EVENTS if leg == "a" else R_EVENT_LIST) | B.R_TOK_BYTE_BLK | B.R_CSR | B.R_STATUS


def pipeline_rates(tok, name, legs, reps, say):
    import datok_amd
    from datok_amd import corpus
    n_docs, doc_bytes = CORPORA[name]
    inputs = [corpus.german_docs(n_docs, doc_bytes, seed=2 + k) for k in range(3)]
    total = int(inputs[0][1][-1])
    pin = datok_amd.PinnedBuffer(total * SLICES)
    for i in range(SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(SLICES)])
    seen = {"bytes": 0, "entries": 0, "bound": 0, "sum": 0}

    def on_slice(leg):
        def cb(first, n, bb):
            t = bb.totals()
            res = bb.result(copy=False)       # host pointers into the slice's page-locked buffers
            nt = t["n_tokens"]
            assert len(res.tok_bblk) == nt and len(res.doc_tail) == n, (leg, len(res.tok_bblk), nt)
            down = 4 * nt + 16 * len(res.tok_bblk_head) + 8 + 24 * (n + 1) + 4 * n + 4 * n   # blocks + flags, CSR, status, tail
            if leg == "a":
                assert res.ev_bits.shape[1] > 0 and len(res.evl_off) == 0
                down += res.ev_bits.size * 4
                seen["sum"] += int(res.ev_bits[2, 0])
            else:
                assert res.ev_bits.shape[1] == 0 and len(res.evl_off) == n + 1   # (the form asked for, not a stand-in)
                bound = t["n_sent"] + t["n_texts"]
                assert len(res.evl_pos) <= bound
                down += 5 * bound + 4 * (n + 1) + 4        # the copies are sized for the bound; the count word
                seen["entries"] += len(res.evl_pos)
                seen["bound"] += bound
                seen["sum"] += int(res.evl_off[-1])
            seen["bytes"] += down
        return cb
    pipes = {}
    for leg in legs:
        pipes[leg] = datok_amd.Pipeline(total, n_docs, depth=DEPTH)
        pipes[leg].set_result_fields(fields(leg))
        pipes[leg].run(tok, pin.array, big_off, RUN_FLAGS, on_slice(leg))   # allocations, lane plans, page-locked buffers
    rates = {leg: [] for leg in legs}
    extra = {}
    for rep in range(reps):
        for leg in legs:
            seen.update(bytes=0, entries=0, bound=0)
            t0 = time.perf_counter()
            pipes[leg].run(tok, pin.array, big_off, RUN_FLAGS, on_slice(leg))
            rates[leg].append(total * SLICES / (time.perf_counter() - t0) / 1e9)
            extra[leg] = dict(seen)
    for p in pipes.values():
        p.close()
    pin.close()
    for leg in legs:
        v = sorted(rates[leg])
        line = {"corpus": name, "docs_per_slice": n_docs, "doc_bytes": doc_bytes, "leg": leg,
                "down_B_per_input_byte": round(extra[leg]["bytes"] / (total * SLICES), 3),
                "GBps_median": round(v[len(v) // 2], 2), "GBps_min": round(v[0], 2), "GBps_max": round(v[-1], 2), "runs": len(v)}
        if leg == "b":
            line.update(entries=extra[leg]["entries"], bound=extra[leg]["bound"],
                        entries_B_per_input_byte=round(5 * extra[leg]["entries"] / (total * SLICES), 4))
        say(json.dumps(line))
    return {leg: sorted(v) for leg, v in rates.items()}, inputs[0]


class _EvListArgs(C.Structure):   # DtkEvListArgs, dtk_internal.h
    _fields_ = [("bits", C.c_void_p), ("bit_words", C.c_uint32), ("n_docs", C.c_uint32), ("doc_off", C.c_void_p),
                ("n_bits", C.c_uint64), ("n_tiles", C.c_uint32), ("cap", C.c_uint32), ("tile_base", C.c_void_p),
                ("count", C.c_void_p), ("evl_off", C.c_void_p), ("evl_pos", C.c_void_p), ("evl_kind", C.c_void_p),
                ("evl_bit", C.c_void_p)]


def kernel_times(tok, text, off, say, launches=20):
    """The four kernels of dtk_launch_evlist on the bitmaps of one slice, microseconds per launch of all four."""
    import datok_amd
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_input(text, off)
        b.run(tok, RUN_FLAGS)
        t = b.totals()
        v = b.result_device()
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        n_docs, cap = len(off) - 1, t["n_sent"] + t["n_texts"]
        n_bits = int(off[-1]) + n_docs
        L.dtk_evlist_tiles.argtypes, L.dtk_evlist_tiles.restype = [C.c_uint64, C.c_uint32], C.c_uint32
        L.dtk_launch_evlist.argtypes = [C.POINTER(_EvListArgs), C.c_void_p]
        tiles = L.dtk_evlist_tiles(n_bits, int(v.ev_words))
        sizes = {"doc_off": 8 * (n_docs + 1), "tile_base": 4 * max(tiles, 1), "count": 4, "evl_off": 4 * (n_docs + 1),
                 "evl_pos": 4 * cap, "evl_kind": cap, "evl_bit": 4 * cap}
        mem = {}
        for k, n in sizes.items():
            mem[k] = C.c_void_p()
            ok(hip.hipMalloc(C.byref(mem[k]), C.c_size_t(max(n, 4))))
        d_off = np.ascontiguousarray(off, dtype=np.uint64)
        ok(hip.hipMemcpy(mem["doc_off"], C.c_void_p(d_off.ctypes.data), C.c_size_t(sizes["doc_off"]), 1))   # host to device
        a = _EvListArgs(v.ev_bits, int(v.ev_words), n_docs, mem["doc_off"], n_bits, tiles, cap, mem["tile_base"],
                        mem["count"], mem["evl_off"], mem["evl_pos"], mem["evl_kind"], mem["evl_bit"])
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        us = []
        for rep in range(4):                      # (the first round is the warm-up)
            ok(hip.hipEventRecord(e0, stream))
            for _ in range(launches):
                ok(L.dtk_launch_evlist(C.byref(a), stream))
            ok(hip.hipEventRecord(e1, stream))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if rep:
                us.append(ms.value * 1e3 / launches)
        count = np.zeros(1, dtype=np.uint32)
        ok(hip.hipMemcpy(C.c_void_p(count.ctypes.data), mem["count"], C.c_size_t(4), 2))                    # device to host
        for p in mem.values():
            ok(hip.hipFree(p))
        ok(hip.hipEventDestroy(e0))
        ok(hip.hipEventDestroy(e1))
    say(json.dumps({"evlist_us_per_launch": round(sorted(us)[len(us) // 2], 2), "kernels": 4, "tiles": tiles,
                    "bitmap_words_per_kind": int(v.ev_words), "entries": int(count[0]), "bound": cap,
                    "launches_per_sample": launches,
                    "what": "k_evl_count + k_evl_scan + k_evl_write + k_evl_rows back to back on the download stream, "
                            "between two HIP events; three bitmaps read twice"}))


def child(args):
    import datok_amd
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    datok_amd.lib().dtk_set_device(0)
    tok = datok_amd.load_tokenizer_file(MODEL)
    assert tok is not None
    say(json.dumps({"library": os.path.relpath(datok_amd._lib.LIB_PATH, ROOT), "legs": args.legs}))
    rates = {}
    for name in CORPORA:
        rates[name], one = pipeline_rates(tok, name, args.legs, args.reps, say)
        if name == "4k" and "b" in args.legs:
            kernel_times(tok, one[0], one[1], say)
    if "a" in args.legs and "b" in args.legs:
        for name, r in rates.items():
            say("corpus %s: list / bitmaps = %.3f at the median;  slowest run of b %.2f GB/s, fastest run of a %.2f GB/s: %s"
                % (name, r["b"][len(r["b"]) // 2] / r["a"][len(r["a"]) // 2], r["b"][0], r["a"][-1],
                   "a gain" if r["b"][0] > r["a"][-1] else "NO gain beyond the spread"))
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="ab", choices=["ab", "a", "b"])
    ap.add_argument("--out", default=None, help="also write the raw lines and the summary to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--legs", args.legs]
    cmd += (["--out", args.out] if args.out else []) + (["--append"] if args.append else [])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_") or k == "DATOK_GPU_LIB"}
    return subprocess.run(cmd, env=env, timeout=900).returncode


if __name__ == "__main__":
    sys.exit(main())
