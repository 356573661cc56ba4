#!/usr/bin/env python3
"""What a tokenizer with more than 255 distinct symbol-stream entries costs: the lean loop over 16-bit entries against
the lean loop over codes and against the general loop such a model took before.

The bench batch (corpus.german_docs, 4096 x 4 KiB; three batches in flight and one alone), timed as bench.py's
timed_steps does -- run + totals, warm-up first -- every leg in a fresh child process, the legs alternated and repeated:

  a   tokenizer_de.matok                  codes, lean loop (the headline path)
  a2  ... with 53 more sigma characters   still codes (255 of 255), a table nearly as wide as b's: the fair comparison
  b   ... with 64 more sigma characters   16-bit entries, lean loop
  c   ... and DATOK_GENERAL16=1           16-bit entries, general loop: the path the model took before
  c'  b's model on another build of the library (--parent-lib: the parent commit's), which knows no such switch
  bX  b's model on yet another build (--alt-lib X=path; a build with another row length, say)

The results of b and c on the first batch are compared with each other, array by array.  After the timed steps every
child runs a few batches with the stage events on and reports the symboliser's and the walk's kernel times.  One JSON
line per child, then the summary: median and spread (min .. max) of the milliseconds per batch, c / b, b / a2, c / c'.

usage: python scripts/big_sigma.py [--reps 3] [--steps 60] [--warmup 60] [--parent-lib path] [--out profiles/big_sigma.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RUN_FLAGS = 256 | 512     # bench.py's: offsets only, rune offsets
FIELDS = ("tok_off", "sent_off", "text_off", "tok_rstart", "tok_rend", "sent", "text_tok_end", "text_sent_end", "status")

LEGS = {  # leg -> (model file, environment, what)
    "a": ("de.matok", {}, "codes, lean loop"),
    "a2": ("de53.matok", {}, "+53 characters: codes, lean loop"),
    "b": ("de64.matok", {}, "+64 characters: 16-bit entries, lean loop"),
    "c": ("de64.matok", {"DATOK_GENERAL16": "1"}, "+64 characters: 16-bit entries, general loop"),
}


def timed_steps(batches, tok, steps):
    """bench.py's timed_steps: a batch is completed on the host before it is run again and at the end."""
    for bb in batches:
        bb.sync()
    t0 = time.perf_counter()
    ran = [False] * len(batches)
    for i in range(steps):
        k = i % len(batches)
        if ran[k]:
            batches[k].totals()
        batches[k].run(tok, RUN_FLAGS)
        ran[k] = True
    for k, bb in enumerate(batches):
        if ran[k]:
            bb.totals()
    return time.perf_counter() - t0


def child(args):
    import datok_amd
    tok = datok_amd.load_tokenizer_file(args.model)
    assert tok is not None
    inputs = []
    for k in range(3):
        z = np.load(os.path.join(args.work, "german%d.npz" % k))
        inputs.append((z["text"], z["off"]))
    batches = []
    for text, off in inputs:
        bb = datok_amd.Batch(len(text), len(off) - 1)
        bb.set_input(text, off)
        batches.append(bb)
    tot = None
    for bb in batches:
        bb.run(tok, RUN_FLAGS)
        tot = tot or bb.totals()
    assert tot["n_flagged"] == 0, tot
    if args.dump:
        res = batches[0].result()
        np.savez(args.dump, **{f: np.asarray(getattr(res, f)) for f in FIELDS})
    out = {"leg": args.leg, "sigma_count": tok.info["sigma_count"], "stream_codes": tok.info["stream_codes"],
           "lean_walk": tok.info.get("lean_walk"), "tokens": int(tot["n_tokens"]), "lanes": int(tot["n_lanes"]),
           "repair_rounds": int(tot["repair_rounds"])}
    total = len(inputs[0][0])
    for name, bs in (("three", batches), ("one", batches[:1])):
        timed_steps(bs, tok, args.warmup)
        e = timed_steps(bs, tok, args.steps)
        out["ms_" + name] = round(e / args.steps * 1e3, 4)
        out["gbs_" + name] = round(total * args.steps / e / 1e9, 1)
    # the kernels' own times (HIP events around the stages, one batch alone): medians of 15 runs
    bb = batches[0]
    bb.set_profiling(True)
    rows = []
    for _ in range(15):
        bb.run(tok, RUN_FLAGS)
        bb.totals()
        rows.append(bb.stage_ms())
    out["stage_us"] = {k: round(float(np.median([r[k] for r in rows])) * 1e3, 1) for k in rows[0] if any(r[k] for r in rows)}
    for bb in batches:
        bb.close()
    print(json.dumps(out), flush=True)


def prepare(work):
    import bigsigma
    from datok_amd import corpus
    for name, blob in (("de.matok", bigsigma.read_model("tokenizer_de.matok")), ("de53.matok", bigsigma.enlarged_de(53)),
                       ("de64.matok", bigsigma.enlarged_de(64))):
        with open(os.path.join(work, name), "wb") as f:
            f.write(blob)
    for k in range(3):
        text, off = corpus.german_docs(4096, 4096, seed=2 + k)
        np.savez(os.path.join(work, "german%d.npz" % k), text=text, off=off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None, help="also write the raw lines and the summary to this file")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit: leg c'")
    ap.add_argument("--alt-lib", action="append", default=[], help="NAME=path: leg bNAME, b's model on that build")
    ap.add_argument("--legs", default="a,a2,b,c")
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--model"), ap.add_argument("--work"), ap.add_argument("--dump")
    args = ap.parse_args()
    if args.leg:
        return child(args)

    legs = dict(LEGS)
    order = [l for l in args.legs.split(",") if l]
    if args.parent_lib:
        legs["c'"] = ("de64.matok", {"DATOK_GPU_LIB": os.path.abspath(args.parent_lib)}, "+64 characters on the parent commit's build")
        order.append("c'")
    for spec in args.alt_lib:
        name, path = spec.split("=", 1)
        legs["b" + name] = ("de64.matok", {"DATOK_GPU_LIB": os.path.abspath(path)}, "+64 characters, lean loop, build " + name)
        order.append("b" + name)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as work:
        prepare(work)
        runs = {leg: [] for leg in order}
        for rep in range(max(args.reps, 1)):
            for leg in order:
                model, env, _ = legs[leg]
                e = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
                e.update(env)
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--model", os.path.join(work, model),
                       "--work", work, "--steps", str(args.steps), "--warmup", str(args.warmup)]
                if rep == 0 and leg in ("b", "c"):
                    cmd += ["--dump", os.path.join(work, "res_%s.npz" % leg)]
                r = subprocess.run(cmd, capture_output=True, env=e, timeout=300)
                if r.returncode != 0:
                    say("leg %s rep %d FAILED (%d): %s" % (leg, rep, r.returncode, r.stderr.decode()[-800:]))
                    if args.out:
                        with open(args.out, "w") as f:
                            f.write("\n".join(lines) + "\n")
                    return 1          # (nothing more is started on the GPU behind a failure)
                row = json.loads(r.stdout.decode().strip().splitlines()[-1])
                row["rep"] = rep
                runs[leg].append(row)
                say(json.dumps(row))
        rc = 0
        if "b" in runs and "c" in runs:
            rb, rc_ = np.load(os.path.join(work, "res_b.npz")), np.load(os.path.join(work, "res_c.npz"))
            same = all(np.array_equal(rb[f], rc_[f]) for f in FIELDS)
            say("parity b == c on the first batch, %d arrays, %d tokens: %s" % (len(FIELDS), len(rb["tok_rstart"]), "ok" if same else "MISMATCH"))
            rc |= 0 if same else 1
    for key in ("ms_three", "ms_one"):
        med = {}
        for leg, rows in runs.items():
            v = sorted(r[key] for r in rows)
            med[leg] = (v[len(v) // 2], v[0], v[-1])
            say("%-8s %-3s median %.4f ms  (%.4f .. %.4f)  %s" % (key, leg, med[leg][0], v[0], v[-1], legs[leg][2]))
        if "b" in med and "c" in med:
            ok = med["b"][2] < med["c"][1]          # the slowest run of the new loop beats the fastest of the old one
            say("%-8s c / b = %.2f  required: b faster than c by more than the spread: %s" % (key, med["c"][0] / med["b"][0], "yes" if ok else "NO"))
            rc |= 0 if ok else 2
        if "b" in med and "a2" in med:
            say("%-8s b / a2 = %.3f  (recorded, not fixed in advance)" % (key, med["b"][0] / med["a2"][0]))
        if "a2" in med and "a" in med:
            say("%-8s a2 / a = %.3f" % (key, med["a2"][0] / med["a"][0]))
        if "c" in med and "c'" in med:
            lo, hi = max(med["c"][1], med["c'"][1]), min(med["c"][2], med["c'"][2])
            say("%-8s c / c' = %.3f  spreads overlap: %s" % (key, med["c"][0] / med["c'"][0], "yes" if lo <= hi else "no"))
    for leg, rows in runs.items():
        keys = rows[0]["stage_us"].keys()
        say("stage_us %-3s %s" % (leg, "  ".join("%s %.1f" % (k, float(np.median([r["stage_us"].get(k, 0.0) for r in rows]))) for k in keys)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
