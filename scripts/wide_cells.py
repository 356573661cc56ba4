#!/usr/bin/env python3
"""What a tokenizer of 32 767 states and more costs: the 64-bit fused cells against the 32-bit ones and against the
path such a model took before them.

The bench batch (corpus.german_docs, 4096 x 4 KiB; three batches in flight and one alone), timed as bench.py's
timed_steps does -- run + totals, warm-up first -- every leg in a fresh child process, the legs alternated and repeated:

  a  tokenizer_de.matok                            32-bit fused cells, lean loop (the headline path)
  b  the same model widened to 40 000 states       64-bit fused cells, lean loop
  c  ... with DATOK_NO_FUSED=1                     plain 32-bit cells, general loop: the path it took before
  d  the 65 541-state trie tokenizer as .datok     dense layout in 64-bit fused cells, lean loop
  e  ... with DATOK_NO_DENSE=1                     the file's {base, check} pairs, general loop: the path it took before
     (d, e on a corpus of words over the crafted alphabet)

The results of b and c on the first batch are compared with each other, array by array.  One JSON line per child,
then the summary: median and spread (min .. max) of the milliseconds per batch, b / a, c / b, e / d.

usage: python scripts/wide_cells.py [--reps 3] [--steps 60] [--warmup 60] [--out profiles/wide_cells.txt]
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
MODELS = os.path.join(ROOT, "tests", "golden", "models")
RUN_FLAGS = 256 | 512     # bench.py's: offsets only, rune offsets
FIELDS = ("tok_off", "sent_off", "text_off", "tok_rstart", "tok_rend", "sent", "text_tok_end", "text_sent_end", "status")

LEGS = {  # leg -> (model file, corpus, environment)
    "a": ("tokenizer_de.matok", "german", {}),
    "b": ("wide40000.matok", "german", {}),
    "c": ("wide40000.matok", "german", {"DATOK_NO_FUSED": "1"}),
    "d": ("trie.datok", "words", {}),
    "e": ("trie.datok", "words", {"DATOK_NO_DENSE": "1"}),
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
        z = np.load(os.path.join(args.work, "%s%d.npz" % (args.corpus, k)))
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
    out = {"leg": args.leg, "entry_bytes": tok.info["entry_bytes"], "dense_states": tok.info["dense_states"],
           "state_count": tok.info["state_count"], "device_mb": round(tok.info["device_bytes"] / 1e6, 1),
           "tokens": int(tot["n_tokens"]), "lanes": int(tot["n_lanes"]), "repair_rounds": int(tot["repair_rounds"])}
    total = len(inputs[0][0])
    for name, bs in (("three", batches), ("one", batches[:1])):
        timed_steps(bs, tok, args.warmup)
        e = timed_steps(bs, tok, args.steps)
        out["ms_" + name] = round(e / args.steps * 1e3, 4)
        out["gbs_" + name] = round(total * args.steps / e / 1e9, 1)
    for bb in batches:
        bb.close()
    print(json.dumps(out), flush=True)


def prepare(work):
    import wide
    from datok_amd import corpus
    with open(os.path.join(MODELS, "tokenizer_de.matok"), "rb") as f:
        de = f.read()
    for name, blob in (("tokenizer_de.matok", de), ("wide40000.matok", wide.widen_matok(de, 40000)),
                       ("trie.datok", wide.trie_model("datok"))):
        with open(os.path.join(work, name), "wb") as f:
            f.write(blob)
    for k in range(3):
        text, off = corpus.german_docs(4096, 4096, seed=2 + k)
        np.savez(os.path.join(work, "german%d.npz" % k), text=text, off=off)
        text, off = corpus.concat_docs(wide.word_documents(np.random.default_rng(40 + k), 4096, 4096))
        np.savez(os.path.join(work, "words%d.npz" % k), text=text, off=off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--out", default=None, help="also write the raw lines and the summary to this file")
    ap.add_argument("--legs", default="abcde")
    ap.add_argument("--leg", help="(internal) run one leg in this process")
    ap.add_argument("--model"), ap.add_argument("--corpus"), ap.add_argument("--work"), ap.add_argument("--dump")
    args = ap.parse_args()
    if args.leg:
        return child(args)

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as work:
        prepare(work)
        runs = {leg: [] for leg in args.legs}
        for rep in range(max(args.reps, 1)):
            for leg in args.legs:
                model, corp, env = LEGS[leg]
                e = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_") or k == "DATOK_GPU_LIB"}
                e.update(env)
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--model", os.path.join(work, model),
                       "--corpus", corp, "--work", work, "--steps", str(args.steps), "--warmup", str(args.warmup)]
                if rep == 0 and leg in "bc":
                    cmd += ["--dump", os.path.join(work, "res_%s.npz" % leg)]
                r = subprocess.run(cmd, capture_output=True, env=e, timeout=300)
                if r.returncode != 0:
                    say("leg %s rep %d FAILED (%d): %s" % (leg, rep, r.returncode, r.stderr.decode()[-800:]))
                    return 1          # (nothing more is started on the GPU behind a failure)
                row = json.loads(r.stdout.decode().strip().splitlines()[-1])
                row["rep"] = rep
                runs[leg].append(row)
                say(json.dumps(row))
        if "b" in runs and "c" in runs:
            rb, rc = np.load(os.path.join(work, "res_b.npz")), np.load(os.path.join(work, "res_c.npz"))
            same = all(np.array_equal(rb[f], rc[f]) for f in FIELDS)
            say("parity b == c on the first batch, %d arrays, %d tokens: %s" % (len(FIELDS), len(rb["tok_rstart"]), "ok" if same else "MISMATCH"))
            if not same:
                return 1
    rc = 0
    for key in ("ms_three", "ms_one"):
        med = {}
        for leg, rows in runs.items():
            v = sorted(r[key] for r in rows)
            med[leg] = (v[len(v) // 2], v[0], v[-1])
            say("%-8s %s  median %.4f ms  (%.4f .. %.4f)  %s" % (key, leg, med[leg][0], v[0], v[-1], LEGS[leg][0] + " " + " ".join(LEGS[leg][2])))
        for slow, fast, what in (("c", "b", "required: b faster than c by more than the spread"),
                                 ("e", "d", "required: d faster than e by more than the spread")):
            if slow in med and fast in med:
                ok = med[fast][2] < med[slow][1]          # the slowest run of the new path beats the fastest of the old
                say("%-8s %s / %s = %.2f  %s: %s" % (key, slow, fast, med[slow][0] / med[fast][0], what, "yes" if ok else "NO"))
                rc |= 0 if ok else 2
        if "a" in med and "b" in med:
            say("%-8s b / a = %.3f  target: within 1.3: %s" % (key, med["b"][0] / med["a"][0], "yes" if med["b"][0] <= 1.3 * med["a"][0] else "missed"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
