#!/usr/bin/env python3
"""One long stream through dtk_stream_run against the same bytes as 4 KiB documents through dtk_pipeline_run.

Leg 1 (stream): a single stream of --gib GiB from a cyclic reader -- once bare running text, once with an EOT every 4 KiB
-- through dtk_stream_run with R_TOK_BYTE_BLK | R_EVENT_LIST | R_CSR | R_STATUS, with an empty slice callback and with
dtk_stream_transduce in mode 3 (the C++ replay of every slice into a TOKENS | SENTENCES writer when profiles/stream.txt
was taken; the bytes the device renders since dtk_stream_set_render -- scripts/stream_render.py measures both).
Leg 2 (pipeline): the same bytes as 4 KiB documents through dtk_pipeline_run with the same fields and slice size, on the
same session.  Legs alternate; medians of --reps runs.  Reports both rates, their ratio, and the stream's token count
against the oracle's (one period and two periods of the cyclic text: the count of N periods follows).  No threshold.

The measuring runs in a child process that never imports torch.
usage: python scripts/stream_throughput.py [--gib 1] [--reps 3] [--slice-mib 16] [--out profiles/stream.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODEL = os.path.join(ROOT, "tests", "golden", "models", "tokenizer_de.matok")
PERIOD = 4 << 20          # bytes of the cyclic text: 1024 documents of 4 KiB


def period_text(eot):
    import numpy as np
    from datok_amd import corpus
    text, off = corpus.german_docs(PERIOD // 4096, 4096, seed=17)
    raw = bytearray(bytes(text))
    if eot:   # every document ends in blank + EOT (the blank keeps the last word whole)
        a = np.frombuffer(raw, dtype=np.uint8)
        a[4094::4096] = 0x20
        a[4095::4096] = 0x04
    return bytes(raw)


class Cyclic:
    """A reader that hands out `total` bytes of the period, over and over, straight into the caller's buffer."""

    def __init__(self, period, total):
        self.p, self.n, self.total, self.at = period, len(period), total, 0
        self.addr = C.cast(C.c_char_p(period), C.c_void_p).value

    def fn(self):
        def rd(_u, buf, cap):
            k = min(cap, self.total - self.at, self.n - self.at % self.n)
            if k <= 0:
                return 0
            C.memmove(buf, self.addr + self.at % self.n, k)
            self.at += k
            return k
        return rd


def child(args):
    import numpy as np
    import datok_amd
    from datok_amd import _lib, host
    from oracle import oracle as O
    assert "torch" not in sys.modules
    L = datok_amd.lib()
    B = host.Batch
    fields = B.R_TOK_BYTE_BLK | B.R_EVENT_LIST | B.R_CSR | B.R_STATUS
    tok = datok_amd.load_tokenizer_file(MODEL)
    om = O.Model(MODEL)
    total = int(args.gib * (1 << 30)) // PERIOD * PERIOD
    n_per = total // PERIOD
    S = args.slice_mib << 20
    out = {"bytes": total, "slice_bytes": S, "reps": args.reps, "legs": {}}
    st = host.Stream(S, depth=3)
    st.set_result_fields(fields)
    pipe = host.Pipeline(S, S // 4096 + 8, depth=3)
    pipe.set_result_fields(fields)
    for kind in ("bare", "eot"):
        per = period_text(kind == "eot")
        c1 = om.count_batch(np.frombuffer(per, np.uint8), np.array([0, len(per)], np.uint64))[0, 0]
        c2 = om.count_batch(np.frombuffer(per + per, np.uint8), np.array([0, 2 * len(per)], np.uint64))[0, 0]
        oracle_tokens = int(c1) + (n_per - 1) * int(c2 - c1)
        pin = host.PinnedBuffer(total)
        view = pin.array
        for i in range(n_per):
            view[i * PERIOD:(i + 1) * PERIOD] = np.frombuffer(per, np.uint8)
        doc_off = np.arange(0, total + 1, 4096, dtype=np.uint64)
        times = {"stream": [], "stream_replay": [], "pipeline": []}
        counts = {}
        for rep in range(args.reps + 1):            # (the first round warms up and is dropped)
            n_tok = [0]

            def on_slice(_u, p):
                s = p.contents
                n_tok[0] += int(C.cast(s.view.tok_off, C.POINTER(C.c_uint64))[1])
                return 0
            status = C.c_uint32(0)
            t0 = time.perf_counter()
            rc = L.dtk_stream_run(st._h, tok._h, _lib.READ_FN(Cyclic(per, total).fn()), None, 0, _lib.STREAM_SLICE_FN(on_slice),
                                  None, C.byref(status))
            t1 = time.perf_counter()
            assert rc == 0 and status.value == 0, (rc, status.value)
            counts["stream"] = n_tok[0]
            o, n, s2 = C.c_void_p(), C.c_size_t(), C.c_uint32()
            t2 = time.perf_counter()
            rc = L.dtk_stream_transduce(st._h, tok._h, _lib.READ_FN(Cyclic(per, total).fn()), None, 3, C.byref(o), C.byref(n),
                                        C.byref(s2))
            t3 = time.perf_counter()
            assert rc == 0, rc
            counts["replay_bytes"] = n.value
            L.dtk_free(o)
            ptok = [0]

            def on_docs(first, nd, b):
                ptok[0] += b.totals()["n_tokens"]
            t4 = time.perf_counter()
            pipe.run(tok, view, doc_off, 0, on_docs)
            t5 = time.perf_counter()
            counts["pipeline"] = ptok[0]
            if rep:
                times["stream"].append(t1 - t0); times["stream_replay"].append(t3 - t2); times["pipeline"].append(t5 - t4)
        med = {k: statistics.median(v) for k, v in times.items()}
        out["legs"][kind] = {
            "stream_GBps": total / med["stream"] / 1e9, "stream_replay_GBps": total / med["stream_replay"] / 1e9,
            "pipeline_GBps": total / med["pipeline"] / 1e9, "stream_over_pipeline": med["pipeline"] / med["stream"],
            "seconds": times, "stream_tokens": counts["stream"], "oracle_tokens": oracle_tokens,
            "pipeline_tokens_of_4k_documents": counts["pipeline"], "replay_bytes": counts["replay_bytes"]}
        pin.close()
    # where a slice's time goes: one slice-sized batch alone, stage by stage
    per = period_text(False)
    n = S + 8192
    one = (per * (n // len(per) + 1))[:n]
    with host.Batch(n, 1) as b:
        b.set_profiling(True)
        b.set_input(np.frombuffer(one, np.uint8), np.array([0, n], np.uint64))
        for _ in range(3):
            b.run(tok, host.NO_RUNE_OFFSETS)
            b.totals()
        out["one_slice_stage_ms"] = {"bytes": n, **b.stage_ms()}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice-mib", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--gib", str(args.gib), "--reps", str(args.reps),
           "--slice-mib", str(args.slice_mib)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_") or k == "DATOK_GPU_LIB"}
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=1100)
    line = r.stdout.decode().strip().split("\n")[-1] if r.stdout else ""
    print(line)
    if args.out and r.returncode == 0:
        with open(args.out, "a") as f:
            f.write("stream_throughput.py --gib %s --reps %d --slice-mib %d\n%s\n" % (args.gib, args.reps, args.slice_mib, line))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
