#!/usr/bin/env python3
"""What a user who wants a stream's rune offsets as DATA receives: the position lines as text against the arrays.

A single stream of --gib GiB from a cyclic reader (scripts/stream_throughput.py's: a 4 MiB period of German text) in
--slice-mib MiB slices at depth 3, tokenizer_de.matok, in a child process that never imports torch.  Every leg brings
R_TOK_BYTE_BLK | R_EVENT_LIST | R_CSR | R_STATUS:

  leg a  the walk alone, an empty slice callback
  leg b  mode 12 (TOKEN_POS | SENTENCE_POS) rendered on the device (dtk_stream_set_position_render) and put together by
         dtk_stream_emit into a write_fn that counts the bytes and discards them: the only device route to the offsets
         before dtk_stream_set_offsets
  leg c  dtk_stream_set_offsets, plain form; the callback calls dtk_stream_offsets and adds up the counts
  leg d  the same, blocked form
  leg e  blocked form beside dtk_stream_set_render(3): the surfaces as text, the offsets as arrays

Legs alternate; median of --reps runs after one warm-up round, with min and max.  Per leg the bytes that cross the link
towards the host for one input byte: the view's arrays (4.25 B per token, 5 B per list row), the rendered bytes, and the
offset arrays as dtk_stream_offsets counts them (16 or 4.375 B per token, 8 B per sent int, 8 B per text row).

Then the chain of dtk_launch_streamoffs alone on one slice's arrays, blocked form: the time of each of its ten launches
between HIP events on the batch's download stream (median of --reps), and the copy of what it leaves.

usage: python scripts/stream_offsets.py [--gib 1] [--reps 3] [--slice-mib 16] [--out profiles/stream_offsets.txt]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
MODEL = os.path.join(ROOT, "tests", "golden", "models", "tokenizer_de.matok")
LAUNCHES = ("k_sp_ent_count (sums)", "k_sp_front_scan 0", "k_sp_ent_count", "k_sp_tok_runes", "k_sp_front_scan 1",
            "k_so_tok_place", "k_so_scan", "k_so_sent", "k_so_text", "k_so_pack64")


def stats(seconds, total):
    return {"GBps_median": round(total / statistics.median(seconds) / 1e9, 3), "GBps_min": round(total / max(seconds) / 1e9, 3),
            "GBps_max": round(total / min(seconds) / 1e9, 3), "seconds": [round(s, 4) for s in seconds]}


def launch_times(tok, S, reps):
    """Microseconds of each launch of dtk_launch_streamoffs for one slice (blocked form), and of the copy of its arrays."""
    import numpy as np
    import datok_amd
    from datok_amd import host
    from stream_render import _EvListArgs, _PosArgs
    from stream_throughput import period_text

    class _OffsArgs(C.Structure):     # DtkStreamOffsArgs, dtk_internal.h (dtk_streamoffs_ws fills the workspace pointers)
        _fields_ = [("front", _PosArgs), ("sent_base", C.c_void_p), ("sent_in", C.c_void_p), ("sent", C.c_void_p),
                    ("sent_cap", C.c_uint64), ("text_cap", C.c_uint64), ("text_tok_end", C.c_void_p),
                    ("text_sent_end", C.c_void_p), ("blocked", C.c_uint32), ("span", C.c_uint32), ("words", C.c_void_p),
                    ("heads", C.c_void_p), ("trailer", C.c_void_p)]
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    per = period_text(False)
    n = S + 8192
    text = np.frombuffer((per * (n // len(per) + 1))[:n], np.uint8)
    off = np.array([0, n], np.uint64)
    TRAILER, N_EV = 80, 11
    with datok_amd.Batch(n, 1) as b:
        b.set_input(text, off)
        b.run(tok, host.NO_RUNE_OFFSETS)
        t = b.totals()
        v = b.result_device()
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        rows, nt = t["n_sent"] + t["n_texts"], t["n_tokens"]
        L.dtk_evlist_tiles.argtypes, L.dtk_evlist_tiles.restype = [C.c_uint64, C.c_uint32], C.c_uint32
        L.dtk_launch_evlist.argtypes = [C.POINTER(_EvListArgs), C.c_void_p]
        L.dtk_streamrender_tiles.argtypes, L.dtk_streamrender_tiles.restype = [C.c_uint64], C.c_uint32
        L.dtk_streamoffs_ws.argtypes, L.dtk_streamoffs_ws.restype = [C.POINTER(_OffsArgs), C.c_void_p], C.c_uint64
        L.dtk_launch_streamoffs.argtypes = [C.POINTER(_OffsArgs), C.c_void_p, C.c_void_p]
        ev_tiles = L.dtk_evlist_tiles(n + 1, int(v.ev_words))
        sent_cap, text_cap, nb = min(nt, 3 * rows + 3) + 2 * rows + 1, rows + 1, (nt + 63) // 64
        oa = _OffsArgs(sent_cap=sent_cap, text_cap=text_cap, blocked=1, span=65535)
        f = oa.front
        f.bits, f.with_tail, f.is_matrix, f.first, f.text_len, f.n_tok = 12, 1, 1, 0, n, nt
        f.tok_bstart, f.tok_bend, f.evl_cap, f.doc_tail = v.tok_bstart, v.tok_bend, rows, v.doc_tail
        f.tok_tiles, f.ent_tiles = L.dtk_streamrender_tiles(nt), L.dtk_streamrender_tiles(rows)
        words = L.dtk_streamoffs_ws(C.byref(oa), None)
        sizes = {"text": n, "doc_off": 16, "tile_base": 4 * max(ev_tiles, 1), "count": 4, "evl_off": 8, "evl_pos": 4 * rows,
                 "evl_kind": rows, "evl_bit": 4 * rows, "ws": 8 * words, "carry": 48, "rstart": 8 * nt, "rend": 8 * nt,
                 "sent": 8 * sent_cap, "ttok": 4 * text_cap, "tsent": 4 * text_cap, "heads": 24 * nb, "words": 4 * nt,
                 "trailer": TRAILER}
        mem = {}
        for k, size in sizes.items():
            mem[k] = C.c_void_p()
            ok(hip.hipMalloc(C.byref(mem[k]), C.c_size_t(max(size, 16))))
        ok(hip.hipMemcpy(mem["text"], C.c_void_p(text.ctypes.data), C.c_size_t(n), 1))          # host to device
        ok(hip.hipMemcpy(mem["doc_off"], C.c_void_p(off.ctypes.data), C.c_size_t(16), 1))
        carry0 = np.array([0, 0, 1, 1, 0, 0], np.uint32)       # {posC 0 (64 bits), sentB, init, pos / sent empty}
        ok(hip.hipMemcpy(mem["carry"], C.c_void_p(carry0.ctypes.data), C.c_size_t(24), 1))
        ea = _EvListArgs(v.ev_bits, int(v.ev_words), 1, mem["doc_off"], n + 1, ev_tiles, rows, mem["tile_base"],
                         mem["count"], mem["evl_off"], mem["evl_pos"], mem["evl_kind"], mem["evl_bit"])
        ok(L.dtk_launch_evlist(C.byref(ea), stream))
        f.text, f.evl_pos, f.evl_kind, f.evl_count = mem["text"], mem["evl_pos"], mem["evl_kind"], mem["count"]
        f.carry_in, f.carry_out = mem["carry"].value, mem["carry"].value + 24
        assert L.dtk_streamoffs_ws(C.byref(oa), mem["ws"]) == words
        f.rstart, f.rend = mem["rstart"], mem["rend"]
        oa.sent, oa.text_tok_end, oa.text_sent_end = mem["sent"], mem["ttok"], mem["tsent"]
        oa.words, oa.heads, oa.trailer = mem["words"], mem["heads"], mem["trailer"]
        events = (C.c_void_p * N_EV)()
        for i in range(N_EV):
            ok(hip.hipEventCreate(C.byref(events, i * C.sizeof(C.c_void_p))))
        per_launch = [[] for _ in LAUNCHES]
        for rep in range(reps + 1):                       # (the first round is the warm-up)
            ok(L.dtk_launch_streamoffs(C.byref(oa), stream, events))
            ok(hip.hipEventSynchronize(C.c_void_p(events[N_EV - 1])))
            for i in range(len(LAUNCHES)):
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(events[i]), C.c_void_p(events[i + 1])))
                if rep:
                    per_launch[i].append(ms.value * 1e3)
        # the copy of what the blocked form brings home: sent and the rows as far as the totals reach, heads, words
        copy_bytes = 8 * (t["n_sent"] + 64) + 8 * (t["n_texts"] + 2) + TRAILER + 24 * nb + 4 * nt
        pinned = C.c_void_p(L.dtk_pinned_alloc(max(8 * nt, 8 * sent_cap)))
        assert pinned.value
        us = []
        for rep in range(reps + 1):
            ok(hip.hipEventRecord(C.c_void_p(events[0]), stream))
            for k, size in (("sent", 8 * (t["n_sent"] + 64)), ("heads", 24 * nb), ("words", 4 * nt)):
                ok(hip.hipMemcpyAsync(pinned, mem[k], C.c_size_t(min(size, sizes[k])), 2, stream))      # device to host
            ok(hip.hipEventRecord(C.c_void_p(events[1]), stream))
            ok(hip.hipEventSynchronize(C.c_void_p(events[1])))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(events[0]), C.c_void_p(events[1])))
            if rep:
                us.append(ms.value * 1e3)
        # the arrays against the oracle's for the slice as one document
        def home(k, count, dt):
            a = np.zeros(count, dt)
            if count:
                ok(hip.hipMemcpy(C.c_void_p(a.ctypes.data), mem[k], C.c_size_t(a.nbytes), 2))
            return a
        tr = home("trailer", TRAILER // 8, np.uint64)
        from oracle import oracle as O
        doc = O.Model(MODEL).transduce_doc(text.tobytes(), 0)
        words_, heads_ = home("words", nt, np.uint32), home("heads", nb, host.HEAD64)
        rs, re = host.unpack_blocked64(words_, heads_)
        same = (int(tr[0]) == nt == len(doc.tok_rstart) and int(tr[1]) == len(doc.sent) and int(tr[2]) == len(doc.text_tok_end)
                and np.array_equal(rs, doc.tok_rstart) and np.array_equal(re, doc.tok_rend)
                and np.array_equal(home("rstart", nt, np.int64), doc.tok_rstart)
                and np.array_equal(home("sent", int(tr[1]), np.int64), doc.sent)
                and np.array_equal(home("ttok", int(tr[2]), np.uint32), doc.text_tok_end)
                and np.array_equal(home("tsent", int(tr[2]), np.uint32), doc.text_sent_end))
        out = {"slice_bytes": n, "tokens": nt, "sent_ints": int(tr[1]), "texts": int(tr[2]), "entries_bound": rows,
               "sent_capacity": sent_cap, "text_capacity": text_cap,
               "launch_us": {name: round(statistics.median(x), 1) for name, x in zip(LAUNCHES, per_launch)},
               "chain_us": round(sum(statistics.median(x) for x in per_launch), 1),
               "copy_us": round(statistics.median(us), 1), "copy_bytes": copy_bytes,
               "copy_bytes_per_input_byte": round(copy_bytes / n, 3), "equals_the_oracles_arrays": bool(same),
               "what": "dtk_launch_streamoffs with an event in front of the chain and behind every launch, on the download "
                       "stream, median of %d; the copy: sent, heads and words to page-locked memory" % reps}
        L.dtk_pinned_free(pinned)
        for p in mem.values():
            ok(hip.hipFree(p))
        for i in range(N_EV):
            ok(hip.hipEventDestroy(C.c_void_p(events[i])))
    return out


def child(args):
    import datok_amd
    from datok_amd import _lib, host
    from stream_throughput import PERIOD, Cyclic, period_text
    assert "torch" not in sys.modules
    L = datok_amd.lib()
    B = host.Batch
    fields = B.R_TOK_BYTE_BLK | B.R_EVENT_LIST | B.R_CSR | B.R_STATUS
    tok = datok_amd.load_tokenizer_file(MODEL)
    total = int(args.gib * (1 << 30)) // PERIOD * PERIOD
    S = args.slice_mib << 20
    per = period_text(False)
    st = host.Stream(S, depth=3)
    st.set_result_fields(fields)
    legs = "abcde"
    times = {k: [] for k in legs}
    link = {}
    for rep in range(args.reps + 1):                # (the first round warms up and is dropped)
        for leg in legs:
            status = C.c_uint32(0)
            st.set_offsets(None)                    # (exclusive with position rendering: off first)
            st.set_position_render(12 if leg == "b" else None)
            st.set_offsets({"c": _lib.SO_PLAIN, "d": _lib.SO_BLOCKED, "e": _lib.SO_BLOCKED}.get(leg))
            st.set_render(3 if leg == "e" else None)
            n = {"tokens": 0, "rows": 0, "out": 0, "emitted": 0, "o_tok": 0, "o_sent": 0, "o_text": 0, "o_blocked": 0}

            def discard(_u, _p, nb):
                n["emitted"] += nb
                return 0
            wr = _lib.WRITE_FN(discard)
            so = _lib.StreamOffs()

            def on_slice(_u, p):
                s = p.contents
                n["tokens"] += int(C.cast(s.view.tok_off, C.POINTER(C.c_uint64))[1])
                n["rows"] += int(C.cast(s.view.evl_off, C.POINTER(C.c_uint32))[1])
                n["out"] += int(s.out_len)
                if leg == "b":
                    return L.dtk_stream_emit(st._h, wr, None)
                if leg in "cde":
                    rc = L.dtk_stream_offsets(st._h, C.byref(so))
                    n["o_tok"] += so.n_tok
                    n["o_sent"] += so.n_sent
                    n["o_text"] += so.n_text
                    n["o_blocked"] += 1 if so.tok_rblk else 0
                    return rc
                return 0
            t0 = time.perf_counter()
            rc = L.dtk_stream_run(st._h, tok._h, _lib.READ_FN(Cyclic(per, total).fn()), None, 0,
                                  _lib.STREAM_SLICE_FN(on_slice), None, C.byref(status))
            t1 = time.perf_counter()
            assert rc == 0 and status.value == 0, (leg, rc, status.value)
            assert leg not in "cde" or n["o_tok"] == n["tokens"]
            if rep:
                times[leg].append(t1 - t0)
            view = 4.25 * n["tokens"] + 5 * n["rows"]
            offs = (4.375 if leg in "de" else 16) * n["o_tok"] + 8 * n["o_sent"] + 8 * n["o_text"]
            link[leg] = {"view": round(view / total, 3), "rendered": round(n["out"] / total, 3),
                         "offsets": round(offs / total, 3), "sum": round((view + n["out"] + offs) / total, 3),
                         "tokens": n["tokens"], "sent_ints": n["o_sent"], "texts": n["o_text"], "emitted_bytes": n["emitted"],
                         "blocked_slices": n["o_blocked"]}
    out = {"bytes": total, "slice_bytes": S, "reps": args.reps,
           "legs": {k: stats(v, total) for k, v in times.items()}, "link_bytes_per_input_byte": link,
           "note": "leg b's `rendered` is the length of out; its copy is the capacity bound, 1.29 x that "
                   "(profiles/stream_positions.txt)"}
    st.close()
    out["launches_one_slice"] = launch_times(tok, S, args.reps)
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
    env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=1500)
    line = r.stdout.decode().strip().split("\n")[-1] if r.stdout else ""
    print(line, flush=True)
    if r.returncode != 0:
        return r.returncode
    if args.out:
        with open(args.out, "a") as f:
            f.write("stream_offsets.py --gib %s --reps %d --slice-mib %d\n%s\n" % (args.gib, args.reps, args.slice_mib, line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
