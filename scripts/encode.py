#!/usr/bin/env python3
"""What packing sentences and documents into model input rows costs (dtk_batch_set_encode), on
the bench batch: 4096 x 4 KiB German documents on tokenizer_de.matok, over the vocabulary of scripts/wordpiece.py that
splits about a fifth of the tokens.

  kernel     per fresh run, on the batch's download stream between HIP events: the run is complete, its split and (for
             the sentence unit) its sentence table are finished and waited for; then the spec is attached and
             dtk_batch_download_begin enqueues the encode alone -- the clear of its counters, the three launches of
             dtk_encode.hip and the copy of the counters.  Median of the samples behind a warm-up.  Configurations:
             SENTENCE max_len 128 and DOCUMENT max_len 512 stride 64, each without and with word_id.  The store
             bandwidth printed is n_rows * max_len * 4 B (twice that with word_id) over the time of ALL THREE launches:
             a lower bound of the write kernel's own.
  pipeline   host text in -> host results out through dtk_pipeline_run from page-locked text, 24 slices of 16 MiB,
             depth 4, the legs alternated (SENTENCE, max_len 128):
             leg rows_home   input_ids, row_len, row_piece0 and unit_row_off come home; the pieces stay in HBM
             leg rows_hbm    the rows stay in HBM (rows_home = 0): what the stage is for
             leg pieces      the route without the feature, first half: the pieces and the sentence table come home
  host       ... second half: the rows of ONE slice packed with numpy on one core from the pieces and the sentence table,
             timed once; they equal the device's.

Nothing is gated.  Everything runs in one child process without torch.

usage: python scripts/encode.py [--reps 5] [--out profiles/encode.txt]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import wordpiece as wp  # noqa: E402  (scripts/wordpiece.py: the corpus' vocabulary)

FLAGS = wp.OFFSETS_ONLY | wp.NO_RUNE_OFFSETS
N_DOCS, DOC_BYTES = wp.N_DOCS, wp.DOC_BYTES
SLICES, DEPTH = 24, 4
CLS, SEP, PAD = 1, 2, 0
CONFIGS = [dict(unit="sentence", max_len=128, stride=0), dict(unit="document", max_len=512, stride=64)]
HBM_TBPS = 8.0   # the MI355X's HBM3E peak


def kernel_times(tok, text, off, vocab, say, samples=20):
    import datok_amd
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        ok(hip.hipEventCreate(C.byref(e)))
    with datok_amd.Batch(len(text), len(off) - 1) as b:
        b.set_result_fields(0)                      # the download is the encode alone
        b.set_input(text, off)
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        b.set_wordpiece(vocab, prefix=wp.PREFIX, pieces_home=False)
        for cfg in CONFIGS:
            for word_ids in (False, True):
                us = []
                for k in range(samples + 3):        # (the first three are the warm-up)
                    b.set_encode(None)
                    b.run(tok, FLAGS)
                    b.pieces(device=True)           # the split has finished
                    if cfg["unit"] == "sentence":
                        b.sentences(device=True)    # ... and the sentence table
                    b.set_encode(cls_id=CLS, sep_id=SEP, pad_id=PAD, word_ids=word_ids, rows_home=False, **cfg)
                    ok(hip.hipEventRecord(ev[0], stream))
                    b.download_begin()              # (enqueues the encode alone)
                    ok(hip.hipEventRecord(ev[1], stream))
                    ok(hip.hipEventSynchronize(ev[1]))
                    ms = C.c_float()
                    ok(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
                    if k >= 3:
                        us.append(ms.value * 1e3)
                v = b.encoded(device=True)
                stored = int(v.n_rows) * int(v.max_len) * 4 * (2 if word_ids else 1)
                med = wp.median(us)
                say(json.dumps(dict(cfg, word_id=word_ids, encode_us_median=round(med, 1), encode_us_min=round(min(us), 1),
                                    encode_us_max=round(max(us), 1), samples=len(us), units=int(v.n_units), rows=int(v.n_rows),
                                    cut_units=int(v.n_cut), tokens=b.totals()["n_tokens"], pieces=int(b.pieces(device=True).n_pieces),
                                    table_bytes=stored, store_GBps_at_least=round(stored / med / 1e3, 1),
                                    share_of_hbm_peak=round(stored / med / 1e6 / HBM_TBPS, 3))))
    for e in ev:
        ok(hip.hipEventDestroy(e))


def numpy_rows(piece_off, piece_id, tok_off, sen_off, sen_tok_end, max_len, stride):
    """The rows of the sentence unit packed on the host, vectorised: (input_ids, row_len)."""
    body, step = max_len - 2, max_len - 2 - stride
    n_docs = len(tok_off) - 1
    doc = np.repeat(np.arange(n_docs), np.diff(sen_off.astype(np.int64)))
    base = tok_off.astype(np.int64)[doc]
    first_row = np.arange(len(doc)) == sen_off.astype(np.int64)[doc]
    ends = sen_tok_end.astype(np.int64)
    t1 = base + ends
    t0 = base + np.where(first_row, 0, np.concatenate([[0], ends[:-1]]))
    po = piece_off.astype(np.int64)
    p0, n = po[t0], po[t1] - po[t0]
    w = np.where(n <= body, 1, 1 + -(-(n - body) // step))
    unit = np.repeat(np.arange(len(doc)), w)
    k = np.arange(len(unit)) - np.repeat(np.cumsum(w) - w, w)
    q0 = p0[unit] + k * step
    length = np.minimum(k * step + body, n[unit]) - k * step
    cols = np.arange(body)
    idx = np.minimum(q0[:, None] + cols[None, :], max(len(piece_id) - 1, 0))
    ids = np.full((len(unit), max_len), PAD, np.int32)
    ids[:, 0] = CLS
    ids[:, 1:1 + body] = np.where(cols[None, :] < length[:, None], piece_id[idx], PAD)
    ids[np.arange(len(unit)), 1 + length] = SEP
    return ids, (length + 2).astype(np.uint32)


def pipeline_rates(tok, inputs, vocab, reps, say):
    import datok_amd
    B = datok_amd.Batch
    cfg = CONFIGS[0]
    total = int(inputs[0][1][-1])
    pin = datok_amd.PinnedBuffer(total * SLICES)
    for i in range(SLICES):
        pin.array[i * total:(i + 1) * total] = inputs[i % 3][0]
    big_off = np.concatenate([inputs[i % 3][1][(1 if i else 0):] + np.uint64(i * total) for i in range(SLICES)])
    seen = {"rows": 0, "sum": 0, "keep": None}

    def cb_rows_home(first, n, bb):
        e = bb.encoded(copy=False)                  # (came home with the slice: this waits, and fetches what the first copies left out)
        seen["rows"] += e.n_rows
        seen["sum"] += int(e.input_ids[-1, 1]) + int(e.row_len[-1])
        if first == 0 and seen["keep"] is None:
            seen["keep"] = (e.input_ids.copy(), e.row_len.copy())

    def cb_rows_hbm(first, n, bb):
        seen["rows"] += int(bb.encoded(device=True).n_rows)

    def cb_pieces(first, n, bb):
        p, s = bb.pieces(copy=False), bb.sentences(copy=False)
        seen["rows"] += int(s.n_sen)
        seen["sum"] += int(p.piece_id[-1]) + int(s.sen_tok_end[-1])
    legs = {}
    for leg, home, cb in (("rows_home", True, cb_rows_home), ("rows_hbm", False, cb_rows_hbm)):
        p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
        p.set_wordpiece(vocab, prefix=wp.PREFIX, pieces_home=False)
        p.set_encode(cls_id=CLS, sep_id=SEP, pad_id=PAD, rows_home=home, **cfg)
        p.set_result_fields(B.R_CSR | B.R_STATUS)
        legs[leg] = (p, cb)
    p = datok_amd.Pipeline(total, N_DOCS, depth=DEPTH)
    p.set_wordpiece(vocab, prefix=wp.PREFIX, pieces_home=True)
    p.set_result_fields(B.R_CSR | B.R_STATUS | B.R_SENTENCES)
    legs["pieces"] = (p, cb_pieces)
    for p, cb in legs.values():
        p.run(tok, pin.array, big_off, FLAGS, cb)   # allocations, lane plans, page-locked buffers
    rates = {leg: [] for leg in legs}
    rows = {}
    for rep in range(reps):
        for leg, (p, cb) in legs.items():           # the legs alternate
            seen.update(rows=0, sum=0)
            t0 = time.perf_counter()
            p.run(tok, pin.array, big_off, FLAGS, cb)
            rates[leg].append(total * SLICES / (time.perf_counter() - t0) / 1e9)
            rows[leg] = seen["rows"]
    for leg, v in rates.items():
        say(json.dumps({"pipeline_leg": leg, "GBps_median": round(wp.median(v), 2), "GBps_min": round(min(v), 2),
                        "GBps_max": round(max(v), 2), "runs": len(v), "slices": SLICES, "depth": DEPTH, "slice_bytes": total,
                        "rows_or_sentences": rows[leg], "unit": cfg["unit"], "max_len": cfg["max_len"]}))
    for p, _ in legs.values():
        p.close()
    pin.close()
    return {leg: wp.median(v) for leg, v in rates.items()}, seen["keep"]


def child(args):
    import datok_amd
    from datok_amd import corpus
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    datok_amd.lib().dtk_set_device(0)
    tok = datok_amd.load_tokenizer_file(wp.MODEL)
    assert tok is not None
    inputs = [corpus.german_docs(N_DOCS, DOC_BYTES, seed=2 + k) for k in range(3)]
    text, off = inputs[0]
    B = datok_amd.Batch
    with B(len(text), N_DOCS) as b:                 # the corpus' surfaces, for the vocabulary
        b.set_input(text, off)
        b.set_result_fields(B.R_TOK_BYTE | B.R_CSR)
        b.run(tok, FLAGS)
        r = b.result()
    freq = collections.Counter(wp.surfaces_of(bytes(text), off, r))
    words, n_whole = wp.build_vocabulary(freq)
    vocab = datok_amd.Vocab(words)
    say(json.dumps({"library": os.path.relpath(datok_amd._lib.LIB_PATH, ROOT), "docs": N_DOCS, "doc_bytes": DOC_BYTES,
                    "vocabulary": len(words), "whole_surfaces": n_whole, "vocabulary_covers": wp.COVER}))
    kernel_times(tok, text, off, vocab, say)
    med, kept = pipeline_rates(tok, inputs, vocab, args.reps, say)
    # the route without the feature, second half: one core, one slice, numpy
    cfg = CONFIGS[0]
    with B(len(text), N_DOCS) as b:
        b.set_input(text, off)
        b.set_wordpiece(vocab, prefix=wp.PREFIX)
        b.set_result_fields(B.R_CSR | B.R_STATUS | B.R_SENTENCES)
        b.run(tok, FLAGS)
        p, s, rr = b.pieces(), b.sentences(), b.result()
    t0 = time.perf_counter()
    ids, row_len = numpy_rows(p.piece_off, p.piece_id, rr.tok_off, s.sen_off, s.sen_tok_end, cfg["max_len"], cfg["stride"])
    host_s = time.perf_counter() - t0
    assert kept is not None and np.array_equal(ids, kept[0]) and np.array_equal(row_len, kept[1]), "the host's rows are the device's"
    rate = len(text) / host_s / 1e9
    say(json.dumps({"numpy_packing_one_slice_s": round(host_s, 3), "numpy_GBps_of_input": round(rate, 3), "rows": len(ids),
                    "what": "input_ids and row_len of one slice from pieces and sentence table, vectorised numpy, one core; "
                            "rows equal the device's"}))
    both = 1 / (1 / med["pieces"] + 1 / rate)
    say("medians GB/s of input: rows home %.2f, rows left in HBM %.2f; without the feature: pieces and sentence table home "
        "%.2f, then the numpy packing at %.3f -- one after the other %.3f" % (med["rows_home"], med["rows_hbm"], med["pieces"], rate, both))
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
