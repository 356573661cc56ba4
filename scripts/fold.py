#!/usr/bin/env python3
"""What folding token keys on the device costs (dtk_batch_set_fold), on the bench batch: 4096 x
4 KiB German documents on tokenizer_de.matok, and what the change costs a run WITHOUT a fold, measured against a build of
the parent commit in the same session, the builds alternated.

  --parent DIR   a checkout of the parent commit with its library built (DIR/datok_amd/libdatok_gpu.so): every round
                 measures it and this tree one after the other, each in a process of its own
  per process    k_token_ids and the three launches of the split, per fresh run between HIP events on the download stream
                 (scripts/wordpiece.py: kernel_times), over the vocabularies of scripts/wordpiece.py -- the most frequent
                 surfaces covering 75 % resp. 99.9 % of the tokens -- with no fold; in this tree also with the empty
                 mapping and with bert_uncased_mapping() over a vocabulary made the same way of the corpus's FOLDED
                 surfaces
  pipeline       host text in -> pieces out through dtk_pipeline_run from page-locked text, 24 slices, depth 4, with the
                 fold on and off, alternated
  host           the one-core alternative to the fold alone: str.lower() and unicodedata.normalize("NFD") without the Mn
                 characters over the same bytes
  bench          python bench.py --gpus 1 of either tree, alternated; the build that goes first changes from round to
                 round (--first), and --bench-only runs nothing else

Nothing is gated.  Everything that touches the GPU runs in child processes without torch, one at a time.

usage: python scripts/fold.py --parent DIR [--reps 3] [--first this] [--bench-only] [--out profiles/fold.txt]
"""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "models", "tokenizer_de.matok")


def child(args):
    """One process: the package of --root (this tree or the parent's) measured; JSON lines on stdout."""
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "scripts"))
    import datok_amd
    import wordpiece as W                          # scripts/wordpiece.py of that tree: the corpus, the vocabulary, the timing
    from datok_amd import corpus
    label = args.label

    def say(s):
        print(s, flush=True)

    def times(vocab, what, fold=None):
        out = []
        if fold is None:
            W.kernel_times(tok, text, off, vocab, out.append, what)
        else:
            # (kernel_times attaches vocabulary and split itself; the fold rides on the batch class for its duration)
            make = datok_amd.Batch

            class Folded(make):
                def __init__(self, *a, **kw):
                    super().__init__(*a, **kw)
                    self.set_fold(fold)
            datok_amd.Batch = Folded
            try:
                W.kernel_times(tok, text, off, vocab, out.append, what)
            finally:
                datok_amd.Batch = make
        d = json.loads(out[0])
        d["build"] = label
        say(json.dumps(d))
        return d
    datok_amd.lib().dtk_set_device(0)
    tok = datok_amd.load_tokenizer_file(MODEL)
    assert tok is not None
    inputs = [corpus.german_docs(W.N_DOCS, W.DOC_BYTES, seed=2 + k) for k in range(3)]
    text, off = inputs[0]
    raw = bytes(text)
    B = datok_amd.Batch
    with B(len(text), W.N_DOCS) as b:
        b.set_input(text, off)
        b.set_result_fields(B.R_TOK_BYTE | B.R_CSR)
        b.run(tok, W.FLAGS)
        r = b.result()
    surf = W.surfaces_of(raw, off, r)
    freq = collections.Counter(surf)
    for cover in (W.COVER, W.COVER_WORDS):
        words, _ = W.build_vocabulary(freq, cover)
        times(datok_amd.Vocab(words), "no fold, vocabulary covers %s" % cover)
    if not hasattr(datok_amd, "Fold"):
        return 0
    words, _ = W.build_vocabulary(freq, W.COVER)
    times(datok_amd.Vocab(words), "the empty mapping, vocabulary covers %s" % W.COVER, fold=datok_amd.Fold({}))
    t0 = time.perf_counter()
    mapping = datok_amd.bert_uncased_mapping()
    say(json.dumps({"bert_uncased_mapping_s": round(time.perf_counter() - t0, 2), "sources": len(mapping)}))
    f = datok_amd.Fold(mapping)
    folded = collections.Counter()
    memo = {}
    for s, n in freq.items():
        memo[s] = "".join(mapping.get(ord(c), c) for c in s.decode("utf-8")).encode("utf-8")
        if memo[s]:
            folded[memo[s]] += n
    changed = sum(n for s, n in freq.items() if memo[s] != s)
    non_ascii = sum(1 for c in raw if c >= 0x80)
    say(json.dumps({"tokens": len(surf), "tokens_the_fold_changes_share": round(changed / len(surf), 4),
                    "non_ascii_bytes_share": round(non_ascii / len(raw), 4), "distinct_surfaces": len(freq),
                    "distinct_folded_surfaces": len(folded)}))
    for cover in (W.COVER, W.COVER_WORDS):
        fwords, _ = W.build_vocabulary(folded, cover)
        fvocab = datok_amd.Vocab(fwords)
        times(fvocab, "bert_uncased_mapping(), folded vocabulary covers %s" % cover, fold=f)
    # host text in -> pieces out, the fold on and off alternated
    fwords, _ = W.build_vocabulary(folded, W.COVER)
    fvocab = datok_amd.Vocab(fwords)
    total = int(off[-1])
    pin = datok_amd.PinnedBuffer(total * W.SLICES)
    import numpy as np
    for i in range(W.SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(W.SLICES)])
    seen = {"pieces": 0}

    def on_slice(first, n, bb):
        seen["pieces"] += bb.pieces(copy=False).n_pieces
    legs = {}
    for name, fold in (("fold on", f), ("fold off", None)):
        p = datok_amd.Pipeline(total, W.N_DOCS, depth=W.DEPTH)
        p.set_wordpiece(fvocab, prefix=W.PREFIX, pieces_home=True)
        p.set_fold(fold)
        p.set_result_fields(B.R_CSR | B.R_STATUS)
        p.run(tok, pin.array, big_off, W.FLAGS, on_slice)     # allocations, lane plans, page-locked buffers
        legs[name] = p
    rates = {name: [] for name in legs}
    for _ in range(args.reps):
        for name, p in legs.items():
            t0 = time.perf_counter()
            p.run(tok, pin.array, big_off, W.FLAGS, on_slice)
            rates[name].append(total * W.SLICES / (time.perf_counter() - t0) / 1e9)
    for name, v in rates.items():
        say(json.dumps({"build": label, "pipeline_pieces_home": name, "GBps_median": round(W.median(v), 2), "GBps_min": round(min(v), 2),
                        "GBps_max": round(max(v), 2), "runs": len(v), "slices": W.SLICES, "depth": W.DEPTH, "slice_bytes": total}))
    for p in legs.values():
        p.close()
    pin.close()
    # the host alternative to the fold alone, one core
    import unicodedata
    t0 = time.perf_counter()
    s = raw.decode("utf-8").lower()
    s = "".join(c for c in unicodedata.normalize("NFD", s) if unicodedata.category(c) != "Mn")
    host_s = time.perf_counter() - t0
    say(json.dumps({"host_lower_nfd_strip_s": round(host_s, 3), "host_GBps": round(len(raw) / host_s / 1e9, 4), "bytes": len(raw),
                    "what": "str.lower(), unicodedata.normalize('NFD') and dropping category Mn over one slice, one core, CPython; "
                            "offsets into the source text are lost"}))
    return 0


def run_child(root, label, reps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--label", label, "--reps", str(reps)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
    env["DATOK_GPU_LIB"] = os.path.join(root, "datok_amd", "libdatok_gpu.so")
    r = subprocess.run(cmd, env=env, timeout=600, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("the %s build's measurement failed (exit %d)" % (label, r.returncode))
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


def run_bench(root, steps, warmup):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       env=env, cwd=root, timeout=600, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit("bench.py of %s failed (exit %d)" % (root, r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=3, help="rounds; each measures both builds")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--bench-only", action="store_true", help="only the bench.py runs")
    ap.add_argument("--first", choices=("parent", "this"), default="parent", help="the build the first round begins with")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    ap.add_argument("--root", default=ROOT, help="(internal)")
    ap.add_argument("--label", default="this", help="(internal)")
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    builds = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", ROOT)]
    kernel = collections.defaultdict(lambda: collections.defaultdict(list))   # what -> build -> [(lookup us, split us)]
    bench = collections.defaultdict(list)
    for rnd in range(args.reps):
        parent_first = (args.first == "parent") == (rnd % 2 == 0)   # (the build that goes first changes from round to round)
        order = sorted(builds, key=lambda b: (b[0] == "parent") != parent_first)
        for label, root in order if not args.bench_only else []:    # the builds alternate
            for d in run_child(root, label, args.reps):
                d["round"] = rnd
                say(json.dumps(d))
                if "split_us_median" in d:
                    kernel[d["vocabulary_covers"]][label].append((d["k_token_ids_us_median"], d["split_us_median"]))
        for label, root in order:
            d = run_bench(root, args.bench_steps, 6)
            bench[label].append(d)
            say(json.dumps({"build": label, "round": rnd, "bench_value_MBps": d["value"], "ms_per_step": d["ms_per_step"]}))
    med = lambda v: sorted(v)[len(v) // 2]
    for what, per in kernel.items():
        for label, v in per.items():
            ids, wp = [a for a, _ in v], [b for _, b in v]
            say("%-60s %-6s lookup us median %.1f (%.1f .. %.1f)   split us median %.1f (%.1f .. %.1f)   over %d processes"
                % (what, label, med(ids), min(ids), max(ids), med(wp), min(wp), max(wp), len(v)))
    for label, v in bench.items():
        key = next((k for k in ("value", "throughput", "gbps", "GBps") if k in v[0]), None)
        if key:
            vals = [float(d[key]) for d in v]
            say("bench.py %-6s %s median %.3f (%.3f .. %.3f) over %d runs" % (label, key, med(vals), min(vals), max(vals), len(vals)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
