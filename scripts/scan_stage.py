"""The scan stage (three-launch path: more than 8192 documents) at 8193 and 32768 documents of 64 B: stage times of
repeated runs, median and minimum."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import datok_amd
from datok_amd import corpus
M = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "models")
tok = datok_amd.load_tokenizer_file(os.path.join(M, "tokenizer_de.matok"))
text, _ = corpus.german_docs(1024, 4096, seed=3)
for n in (8193, 32768):
    off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(64))
    t = text[: n * 64]
    with datok_amd.Batch(len(t), n) as b:
        b.set_input(t, off)
        b.set_profiling(True)
        for _ in range(10):
            b.run(tok, 0); b.sync()
        tok_off = b.result().tok_off.copy()
        xs = []
        for _ in range(200):
            b.run(tok, 0); b.sync()
            xs.append(b.stage_ms()["scan"] * 1e3)
        print("three_all %6d documents of 64 B: scan median %.1f us min %.1f  (tok_off sum %d)" % (
            n, float(np.median(xs)), min(xs), int(tok_off.astype(np.uint64).sum())), flush=True)
