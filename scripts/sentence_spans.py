#!/usr/bin/env python3
"""What the sentence table (DTK_R_SENTENCES) costs a caller that only splits sentences: host text
in -> host results out through dtk_pipeline_run from page-locked text, 24 slices, depth 4, on one machine in one process:

  leg offsets    R_TOK_RUNE | R_SENT | R_CSR | R_STATUS   rune offsets and the flat sentence list (the fields of bench.py's
                 end_to_end.with_results_MBps; run flags OFFSETS_ONLY | NO_BYTE_OFFSETS as there)
  leg sentences  R_SENTENCES | R_CSR | R_STATUS           the sentence table (run flags OFFSETS_ONLY: the table is keyed
                 on tok_bend, so the run writes byte offsets too)
  leg upload     the bare upload of every slice's text, nothing else

  corpus 4k   the bench's 4096 x 4 KiB German documents per slice
  corpus 64k  256 x 64 KiB documents per slice

The legs are alternated and repeated; per leg the GB/s of every timed run (median, min .. max) and the bytes on the link
per input byte (up and down).  Then the time of the table's five kernels on one slice of corpus 4k, with HIP events on
the batch's download stream (the launcher called directly, 20 launches back to back), beside that slice's walk stage.
Nothing is gated.  Everything runs in one child process without torch.

usage: python scripts/sentence_spans.py [--reps 4] [--out profiles/sentence_spans.txt] [--append]
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
OFFSETS_ONLY, NO_BYTE_OFFSETS = 256, 512
SLICES, DEPTH = 24, 4
CORPORA = {"4k": (4096, 4096), "64k": (256, 65536)}
LEGS = ("offsets", "sentences", "upload")


def pipeline_rates(tok, name, reps, say):
    import datok_amd
    from datok_amd import corpus
    B = datok_amd.Batch
    n_docs, doc_bytes = CORPORA[name]
    inputs = [corpus.german_docs(n_docs, doc_bytes, seed=2 + k) for k in range(3)]
    total = int(inputs[0][1][-1])
    pin = datok_amd.PinnedBuffer(total * SLICES)
    for i in range(SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(SLICES)])
    seen = {"down": 0, "rows": 0, "bound": 0, "sum": 0}

    def on_slice(leg):
        def cb(first, n, bb):
            t = bb.totals()
            res = bb.result(copy=False)          # host pointers into the slice's page-locked buffers
            down = 24 * (n + 1) + 4 * n          # CSR, status
            if leg == "offsets":
                assert len(res.tok_rend) == t["n_tokens"] and len(res.sent) == t["n_sent"]
                down += 8 * t["n_tokens"] + 4 * t["n_sent"]
                seen["sum"] += int(res.tok_rend[-1]) + int(res.sent[-1])
            else:
                s = bb.sentences(copy=False)     # (came home with the slice: this only waits)
                assert len(res.tok_rend) == 0 and s.n_sen == int(s.sen_off[-1]) <= t["n_sent"]
                # one copy of the whole block, sized for the bound n_sent: sen_off, five words per row, text rows, count
                down += 8 * (n + 1) + 20 * max(t["n_sent"], 1) + 4 * t["n_texts"] + 4
                seen["rows"] += s.n_sen
                seen["bound"] += t["n_sent"]
                seen["sum"] += int(s.sen_rend[-1]) + int(s.sen_bend[-1])
            seen["down"] += down
        return cb
    pipes = {"offsets": (datok_amd.Pipeline(total, n_docs, depth=DEPTH), B.R_TOK_RUNE | B.R_SENT | B.R_CSR | B.R_STATUS,
                         OFFSETS_ONLY | NO_BYTE_OFFSETS),
             "sentences": (datok_amd.Pipeline(total, n_docs, depth=DEPTH), B.R_SENTENCES | B.R_CSR | B.R_STATUS, OFFSETS_ONLY)}
    for leg, (p, fields, flags) in pipes.items():
        p.set_result_fields(fields)
        p.run(tok, pin.array, big_off, flags, on_slice(leg))   # allocations, lane plans, page-locked buffers
    hb = datok_amd.Batch(total, n_docs)

    def upload():
        for i in range(SLICES):
            hb.set_input(pin.array[i * total:(i + 1) * total], inputs[0][1])
        hb.sync()
    upload()
    rates = {leg: [] for leg in LEGS}
    extra = {}
    for rep in range(reps):
        for leg in LEGS:
            seen.update(down=0, rows=0, bound=0)
            t0 = time.perf_counter()
            if leg == "upload":
                upload()
            else:
                p, fields, flags = pipes[leg]
                p.run(tok, pin.array, big_off, flags, on_slice(leg))
            rates[leg].append(total * SLICES / (time.perf_counter() - t0) / 1e9)
            extra[leg] = dict(seen)
    for p, _, _ in pipes.values():
        p.close()
    hb.close()
    pin.close()
    for leg in LEGS:
        v = sorted(rates[leg])
        up = 1 + 8 * (n_docs + 1) / total
        line = {"corpus": name, "docs_per_slice": n_docs, "doc_bytes": doc_bytes, "leg": leg,
                "up_B_per_input_byte": round(up, 3), "down_B_per_input_byte": round(extra[leg]["down"] / (total * SLICES), 4),
                "GBps_median": round(v[len(v) // 2], 2), "GBps_min": round(v[0], 2), "GBps_max": round(v[-1], 2), "runs": len(v)}
        if leg == "sentences":
            line.update(rows=extra[leg]["rows"], bound=extra[leg]["bound"],
                        rows_B_per_input_byte=round(20 * extra[leg]["rows"] / (total * SLICES), 4))
        say(json.dumps(line))
    return {leg: sorted(v) for leg, v in rates.items()}, inputs[0]


class _SentencesArgs(C.Structure):   # DtkSentencesArgs, dtk_internal.h
    _fields_ = [("bits", C.c_void_p), ("bit_words", C.c_uint32), ("n_docs", C.c_uint32), ("doc_off", C.c_void_p),
                ("n_bits", C.c_uint64), ("n_tiles", C.c_uint32), ("cap", C.c_uint32), ("tok_off", C.c_void_p),
                ("text_off", C.c_void_p), ("tok_bstart", C.c_void_p), ("tok_bend", C.c_void_p), ("tok_rstart", C.c_void_p),
                ("tok_rend", C.c_void_p), ("text_tok_end", C.c_void_p), ("text_cap", C.c_uint64), ("tile_base", C.c_void_p),
                ("tile_in", C.c_void_p), ("count", C.c_void_p), ("sen_bit", C.c_void_p), ("sen_doc", C.c_void_p),
                ("sen_first", C.c_void_p), ("sen_off", C.c_void_p), ("sen_tok_end", C.c_void_p), ("sen_bstart", C.c_void_p),
                ("sen_bend", C.c_void_p), ("sen_rstart", C.c_void_p), ("sen_rend", C.c_void_p), ("text_sen_end", C.c_void_p)]


def kernel_times(tok, text, off, say, launches=20):
    """The five kernels of dtk_launch_sentences on one slice, microseconds per launch of all five, and the slice's walk."""
    import datok_amd
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_profiling(True)
        b.set_input(text, off)
        b.run(tok, OFFSETS_ONLY)
        b.run(tok, OFFSETS_ONLY)
        stages = b.stage_ms()
        t = b.totals()
        v = b.result_device()
        table = b.sentences()
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        n_docs, cap, n_texts = len(off) - 1, max(t["n_sent"], 1), t["n_texts"]
        n_bits = int(off[-1]) + n_docs
        L.dtk_sentences_tiles.argtypes, L.dtk_sentences_tiles.restype = [C.c_uint64, C.c_uint32], C.c_uint32
        L.dtk_launch_sentences.argtypes = [C.POINTER(_SentencesArgs), C.c_void_p]
        tiles = L.dtk_sentences_tiles(n_bits, int(v.ev_words))
        sizes = {"doc_off": 8 * (n_docs + 1), "tile_base": 4 * max(tiles, 1), "tile_in": 4 * max(tiles, 1), "count": 4,
                 "sen_off": 8 * (n_docs + 1), "text_sen_end": 4 * max(n_texts, 1)}
        sizes.update({k: 4 * cap for k in ("sen_bit", "sen_doc", "sen_first", "sen_tok_end", "sen_bstart", "sen_bend",
                                           "sen_rstart", "sen_rend")})
        mem = {}
        for k, n in sizes.items():
            mem[k] = C.c_void_p()
            ok(hip.hipMalloc(C.byref(mem[k]), C.c_size_t(max(n, 8))))
        d_off = np.ascontiguousarray(off, dtype=np.uint64)
        ok(hip.hipMemcpy(mem["doc_off"], C.c_void_p(d_off.ctypes.data), C.c_size_t(sizes["doc_off"]), 1))   # host to device
        a = _SentencesArgs(bits=v.ev_bits, bit_words=int(v.ev_words), n_docs=n_docs, doc_off=mem["doc_off"], n_bits=n_bits,
                           n_tiles=tiles, cap=cap, tok_off=v.tok_off, text_off=v.text_off, tok_bstart=v.tok_bstart,
                           tok_bend=v.tok_bend, tok_rstart=v.tok_rstart, tok_rend=v.tok_rend, text_tok_end=v.text_tok_end,
                           text_cap=n_texts, **{k: mem[k] for k in sizes if k != "doc_off"})
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        us = []
        for rep in range(4):                      # (the first round is the warm-up)
            ok(hip.hipEventRecord(e0, stream))
            for _ in range(launches):
                ok(L.dtk_launch_sentences(C.byref(a), stream))
            ok(hip.hipEventRecord(e1, stream))
            ok(hip.hipEventSynchronize(e1))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            if rep:
                us.append(ms.value * 1e3 / launches)
        count = np.zeros(1, dtype=np.uint32)
        ok(hip.hipMemcpy(C.c_void_p(count.ctypes.data), mem["count"], C.c_size_t(4), 2))                    # device to host
        assert int(count[0]) == table.n_sen
        for p in mem.values():
            ok(hip.hipFree(p))
        ok(hip.hipEventDestroy(e0))
        ok(hip.hipEventDestroy(e1))
    say(json.dumps({"sentences_us_per_launch": round(sorted(us)[len(us) // 2], 2), "kernels": 5, "tiles": tiles,
                    "slice_bytes": int(off[-1]), "rows": int(count[0]), "bound": cap, "launches_per_sample": launches,
                    "walk_stage_us": round(stages["walk"] * 1e3, 1), "all_stages_us": round(sum(stages.values()) * 1e3, 1),
                    "what": "k_sen_count + k_sen_scan + k_sen_write + k_sen_rows + k_sen_gather back to back on the "
                            "download stream, between two HIP events; four bitmaps read twice.  walk_stage_us / "
                            "all_stages_us: the same slice's walk and whole run (stage events, one slice alone)"}))


def child(args):
    import datok_amd
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    datok_amd.lib().dtk_set_device(0)
    tok = datok_amd.load_tokenizer_file(MODEL)
    assert tok is not None
    say(json.dumps({"library": os.path.relpath(datok_amd._lib.LIB_PATH, ROOT), "legs": LEGS, "slices": SLICES, "depth": DEPTH}))
    for name in CORPORA:
        r, one = pipeline_rates(tok, name, args.reps, say)
        med = {leg: v[len(v) // 2] for leg, v in r.items()}
        say("corpus %s, medians GB/s: offsets %.2f, sentences %.2f, upload %.2f;  sentences / offsets = %.3f, sentences / "
            "upload = %.3f;  the sentence leg lies %s" % (
                name, med["offsets"], med["sentences"], med["upload"], med["sentences"] / med["offsets"],
                med["sentences"] / med["upload"],
                "between the other two" if med["offsets"] <= med["sentences"] <= med["upload"] else "NOT between the other two"))
        if name == "4k":
            kernel_times(tok, one[0], one[1], say)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None, help="also write the raw lines and the summary to this file")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    cmd += (["--out", args.out] if args.out else []) + (["--append"] if args.append else [])
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_") or k == "DATOK_GPU_LIB"}
    return subprocess.run(cmd, env=env, timeout=900).returncode


if __name__ == "__main__":
    sys.exit(main())
