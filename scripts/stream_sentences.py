#!/usr/bin/env python3
"""What a user who wants a stream's SENTENCES receives: the sentence rows against the token offsets they would
otherwise be rebuilt from.

A single stream of --gib GiB from a cyclic reader (scripts/stream_throughput.py's: a 4 MiB period of German text) in
--slice-mib MiB slices at depth 3, tokenizer_de.matok, in a child process that never imports torch.  Every leg brings
R_TOK_BYTE_BLK | R_EVENT_LIST | R_CSR | R_STATUS:

  leg a  the walk alone, an empty slice callback
  leg b  dtk_stream_set_offsets, blocked form, alone: the way to the same information before dtk_stream_set_sentences
         (the callback calls dtk_stream_offsets and adds up the counts; the host pass that rebuilds the rows from tok_* and
         sent is NOT run, so the leg is the cheaper half of that route)
  leg c  dtk_stream_set_sentences alone; the callback calls dtk_stream_sentences and adds up the counts
  leg d  both

Legs alternate; median of --reps runs after one warm-up round, with min and max.  Per leg the bytes that cross the link
towards the host for one input byte: the view's arrays (4.25 B per token, 5 B per list row), the offset arrays (4.375 B
per token, 8 B per sent int, 8 B per text row) and the sentence rows (36 B per row, 4 B per text row).

Then the four launches of dtk_launch_streamsens alone on one slice's arrays, behind the offsets chain in the plain form
(dtk_launch_streamoffs, which the rows read): the time of each between HIP events on the batch's download stream (median
of --reps), and the copy of what the unit leaves.

usage: python scripts/stream_sentences.py [--gib 1] [--reps 3] [--slice-mib 16] [--out profiles/stream_sentences.txt]
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
LAUNCHES = ("k_ss_count", "k_ss_scan", "k_ss_write", "k_ss_text")


def stats(seconds, total):
    return {"GBps_median": round(total / statistics.median(seconds) / 1e9, 3), "GBps_min": round(total / max(seconds) / 1e9, 3),
            "GBps_max": round(total / min(seconds) / 1e9, 3), "seconds": [round(s, 4) for s in seconds]}


def launch_times(tok, S, reps):
    """Microseconds of each launch of dtk_launch_streamsens for one slice, of the offsets chain in front of it (plain
    form) and of the copy of the rows."""
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

    class _SensArgs(C.Structure):     # DtkStreamSensArgs, dtk_internal.h (dtk_streamsens_ws fills its two workspace pointers)
        _fields_ = [("front", _PosArgs), ("base", C.c_uint64), ("carry_in", C.c_void_p), ("carry_out", C.c_void_p),
                    ("first_base", C.c_void_p), ("first_mask", C.c_void_p), ("sen_cap", C.c_uint64), ("text_cap", C.c_uint64),
                    ("sen_tok_end", C.c_void_p), ("sen_bstart", C.c_void_p), ("sen_bend", C.c_void_p),
                    ("sen_rstart", C.c_void_p), ("sen_rend", C.c_void_p), ("text_sen_end", C.c_void_p), ("trailer", C.c_void_p)]
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    per = period_text(False)
    n = S + 8192
    text = np.frombuffer((per * (n // len(per) + 1))[:n], np.uint8)
    off = np.array([0, n], np.uint64)
    O_TRAILER, S_TRAILER, O_EV, S_EV = 80, 120, 11, 5
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
        L.dtk_streamsens_ws.argtypes, L.dtk_streamsens_ws.restype = [C.POINTER(_SensArgs), C.c_void_p], C.c_uint64
        L.dtk_launch_streamsens.argtypes = [C.POINTER(_SensArgs), C.c_void_p, C.c_void_p]
        ev_tiles = L.dtk_evlist_tiles(n + 1, int(v.ev_words))
        sent_cap, text_cap, sen_cap = min(nt, 3 * rows + 3) + 2 * rows + 1, rows + 1, min(nt, 3 * rows + 3) + 1
        oa = _OffsArgs(sent_cap=sent_cap, text_cap=text_cap, blocked=0, span=65535)
        f = oa.front
        f.bits, f.with_tail, f.is_matrix, f.first, f.text_len, f.n_tok = 12, 1, 1, 0, n, nt
        f.tok_bstart, f.tok_bend, f.evl_cap, f.doc_tail = v.tok_bstart, v.tok_bend, rows, v.doc_tail
        f.tok_tiles, f.ent_tiles = L.dtk_streamrender_tiles(nt), L.dtk_streamrender_tiles(rows)
        words = L.dtk_streamoffs_ws(C.byref(oa), None)
        sa = _SensArgs(sen_cap=sen_cap, text_cap=text_cap, base=0)
        sa.front.n_tok, sa.front.tok_tiles = nt, f.tok_tiles
        s_words = L.dtk_streamsens_ws(C.byref(sa), None)
        sizes = {"text": n, "doc_off": 16, "tile_base": 4 * max(ev_tiles, 1), "count": 4, "evl_off": 8, "evl_pos": 4 * rows,
                 "evl_kind": rows, "evl_bit": 4 * rows, "ws": 8 * words, "carry": 48, "rstart": 8 * nt, "rend": 8 * nt,
                 "sent": 8 * sent_cap, "ttok": 4 * text_cap, "tsent": 4 * text_cap, "trailer": O_TRAILER,
                 "s_ws": 8 * s_words, "s_carry": 80, "s_trailer": S_TRAILER, "s_tse": 4 * text_cap, "s_tok_end": 4 * sen_cap,
                 "s_bstart": 8 * sen_cap, "s_bend": 8 * sen_cap, "s_rstart": 8 * sen_cap, "s_rend": 8 * sen_cap}
        mem = {}
        for k, size in sizes.items():
            mem[k] = C.c_void_p()
            ok(hip.hipMalloc(C.byref(mem[k]), C.c_size_t(max(size, 16))))
        ok(hip.hipMemcpy(mem["text"], C.c_void_p(text.ctypes.data), C.c_size_t(n), 1))          # host to device
        ok(hip.hipMemcpy(mem["doc_off"], C.c_void_p(off.ctypes.data), C.c_size_t(16), 1))
        carry0 = np.array([0, 0, 1, 1, 0, 0], np.uint32)       # {posC 0 (64 bits), sentB, init, pos / sent empty}
        ok(hip.hipMemcpy(mem["carry"], C.c_void_p(carry0.ctypes.data), C.c_size_t(24), 1))
        ok(hip.hipMemset(mem["s_carry"], 0, C.c_size_t(80)))   # no row is open
        ea = _EvListArgs(v.ev_bits, int(v.ev_words), 1, mem["doc_off"], n + 1, ev_tiles, rows, mem["tile_base"],
                         mem["count"], mem["evl_off"], mem["evl_pos"], mem["evl_kind"], mem["evl_bit"])
        ok(L.dtk_launch_evlist(C.byref(ea), stream))
        f.text, f.evl_pos, f.evl_kind, f.evl_count = mem["text"], mem["evl_pos"], mem["evl_kind"], mem["count"]
        f.carry_in, f.carry_out = mem["carry"].value, mem["carry"].value + 24
        assert L.dtk_streamoffs_ws(C.byref(oa), mem["ws"]) == words
        f.rstart, f.rend = mem["rstart"], mem["rend"]
        oa.sent, oa.text_tok_end, oa.text_sent_end, oa.trailer = mem["sent"], mem["ttok"], mem["tsent"], mem["trailer"]
        C.memmove(C.byref(sa.front), C.byref(oa.front), C.sizeof(_PosArgs))      # the chain's arguments as it was launched
        assert L.dtk_streamsens_ws(C.byref(sa), mem["s_ws"]) == s_words
        sa.carry_in, sa.carry_out, sa.trailer = mem["s_carry"].value, mem["s_carry"].value + 40, mem["s_trailer"]
        sa.sen_tok_end, sa.sen_bstart, sa.sen_bend = mem["s_tok_end"], mem["s_bstart"], mem["s_bend"]
        sa.sen_rstart, sa.sen_rend, sa.text_sen_end = mem["s_rstart"], mem["s_rend"], mem["s_tse"]
        o_events, s_events = (C.c_void_p * O_EV)(), (C.c_void_p * S_EV)()
        for evs, cnt in ((o_events, O_EV), (s_events, S_EV)):
            for i in range(cnt):
                ok(hip.hipEventCreate(C.byref(evs, i * C.sizeof(C.c_void_p))))
        per_launch, chain = [[] for _ in LAUNCHES], []
        for rep in range(reps + 1):                       # (the first round is the warm-up)
            ok(L.dtk_launch_streamoffs(C.byref(oa), stream, o_events))
            ok(L.dtk_launch_streamsens(C.byref(sa), stream, s_events))
            ok(hip.hipEventSynchronize(C.c_void_p(s_events[S_EV - 1])))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(o_events[0]), C.c_void_p(o_events[O_EV - 1])))
            if rep:
                chain.append(ms.value * 1e3)
            for i in range(len(LAUNCHES)):
                ok(hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(s_events[i]), C.c_void_p(s_events[i + 1])))
                if rep:
                    per_launch[i].append(ms.value * 1e3)

        def home(k, count, dt):
            a = np.zeros(count, dt)
            if count:
                ok(hip.hipMemcpy(C.c_void_p(a.ctypes.data), mem[k], C.c_size_t(a.nbytes), 2))
            return a
        tr = home("s_trailer", S_TRAILER // 8, np.uint64)
        n_sen, n_text = int(tr[1]), int(tr[2])
        # the copy of what comes home: the trailer with the text rows, the five arrays as far as the totals reach
        home_rows = min(sen_cap, (t["n_sent"] + t["n_texts"] + 1) // 2 + 64)
        pieces = (("s_trailer", S_TRAILER), ("s_tse", 4 * min(text_cap, t["n_texts"] + 2)), ("s_tok_end", 4 * home_rows),
                  ("s_bstart", 8 * home_rows), ("s_bend", 8 * home_rows), ("s_rstart", 8 * home_rows), ("s_rend", 8 * home_rows))
        copy_bytes = sum(size for _, size in pieces)
        pinned = C.c_void_p(L.dtk_pinned_alloc(max(8 * sen_cap, 64)))
        assert pinned.value
        us = []
        for rep in range(reps + 1):
            ok(hip.hipEventRecord(C.c_void_p(s_events[0]), stream))
            for k, size in pieces:
                ok(hip.hipMemcpyAsync(pinned, mem[k], C.c_size_t(size), 2, stream))      # device to host
            ok(hip.hipEventRecord(C.c_void_p(s_events[1]), stream))
            ok(hip.hipEventSynchronize(C.c_void_p(s_events[1])))
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(s_events[0]), C.c_void_p(s_events[1])))
            if rep:
                us.append(ms.value * 1e3)
        # the rows against the definition on the oracle's calls for the slice as one document
        from oracle import oracle as O
        om = O.Model(MODEL)
        raw = text.tobytes()
        doc = om.transduce_doc(raw, 0)
        firsts, k, open_run, toks = [], 0, False, []
        for c in om.events(raw)[0]:
            if c[0] == 0:
                if not open_run:
                    firsts.append(k)
                open_run = True
                toks.append((c[3], c[4]))
                k += 1
            else:
                open_run = False
        ends = firsts[1:] + [k]
        rs, re = np.asarray(doc.tok_rstart, np.int64), np.asarray(doc.tok_rend, np.int64)
        fi, la = np.array(firsts, np.int64), np.array(ends, np.int64) - 1
        tb = np.array(toks, np.int64).reshape(-1, 2)
        same = (int(tr[0]) == nt == k and n_sen == len(firsts) and n_text == len(doc.text_tok_end)
                and np.array_equal(home("s_tok_end", n_sen, np.uint32), ends)
                and np.array_equal(home("s_bstart", n_sen, np.uint64), tb[fi, 0]) and np.array_equal(home("s_bend", n_sen, np.uint64), tb[la, 1])
                and np.array_equal(home("s_rstart", n_sen, np.int64), rs[fi]) and np.array_equal(home("s_rend", n_sen, np.int64), re[la])
                and home("s_tse", n_text, np.uint32).tolist() == [n_sen] * n_text)
        out = {"slice_bytes": n, "tokens": nt, "rows": n_sen, "texts": n_text, "entries_bound": rows,
               "row_capacity": sen_cap, "text_capacity": text_cap,
               "launch_us": {name: round(statistics.median(x), 1) for name, x in zip(LAUNCHES, per_launch)},
               "unit_us": round(sum(statistics.median(x) for x in per_launch), 1),
               "offsets_chain_plain_us": round(statistics.median(chain), 1),
               "copy_us": round(statistics.median(us), 1), "copy_bytes": copy_bytes,
               "copy_bytes_per_input_byte": round(copy_bytes / n, 4), "equals_the_definition_on_the_oracles_calls": bool(same),
               "what": "dtk_launch_streamoffs (plain form, first event to last) and dtk_launch_streamsens with an event in "
                       "front of the unit and behind every launch, on the download stream, median of %d; the copy: the trailer, "
                       "the text rows and the five row arrays to page-locked memory" % reps}
        L.dtk_pinned_free(pinned)
        for p in mem.values():
            ok(hip.hipFree(p))
        for evs, cnt in ((o_events, O_EV), (s_events, S_EV)):
            for i in range(cnt):
                ok(hip.hipEventDestroy(C.c_void_p(evs[i])))
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
    legs = "abcd"
    times = {k: [] for k in legs}
    link = {}
    for rep in range(args.reps + 1):                # (the first round warms up and is dropped)
        for leg in legs:
            status = C.c_uint32(0)
            st.set_offsets(_lib.SO_BLOCKED if leg in "bd" else None)
            st.set_sentences(leg in "cd")
            n = {"tokens": 0, "rows": 0, "o_tok": 0, "o_sent": 0, "o_text": 0, "s_sen": 0, "s_text": 0, "spans": 0}
            so, ss = _lib.StreamOffs(), _lib.StreamSens()

            def on_slice(_u, p):
                s = p.contents
                n["tokens"] += int(C.cast(s.view.tok_off, C.POINTER(C.c_uint64))[1])
                n["rows"] += int(C.cast(s.view.evl_off, C.POINTER(C.c_uint32))[1])
                rc = 0
                if leg in "bd":
                    rc = L.dtk_stream_offsets(st._h, C.byref(so))
                    n["o_tok"] += so.n_tok
                    n["o_sent"] += so.n_sent
                    n["o_text"] += so.n_text
                if leg in "cd" and rc == 0:
                    rc = L.dtk_stream_sentences(st._h, C.byref(ss))
                    n["s_sen"] += ss.n_sen
                    n["s_text"] += ss.n_text
                    n["spans"] += ss.carry_in.open
                return rc
            t0 = time.perf_counter()
            rc = L.dtk_stream_run(st._h, tok._h, _lib.READ_FN(Cyclic(per, total).fn()), None, 0,
                                  _lib.STREAM_SLICE_FN(on_slice), None, C.byref(status))
            t1 = time.perf_counter()
            assert rc == 0 and status.value == 0, (leg, rc, status.value)
            assert leg not in "bd" or n["o_tok"] == n["tokens"]
            if rep:
                times[leg].append(t1 - t0)
            view = 4.25 * n["tokens"] + 5 * n["rows"]
            offs = 4.375 * n["o_tok"] + 8 * n["o_sent"] + 8 * n["o_text"]
            sens = 36 * n["s_sen"] + 4 * n["s_text"]
            link[leg] = {"view": round(view / total, 3), "offsets": round(offs / total, 3), "sentences": round(sens / total, 3),
                         "sum": round((view + offs + sens) / total, 3), "tokens": n["tokens"], "sent_ints": n["o_sent"],
                         "sentence_rows": n["s_sen"], "texts": n["s_text"] or n["o_text"], "slices_with_a_carried_row": n["spans"]}
    out = {"bytes": total, "slice_bytes": S, "reps": args.reps,
           "legs": {k: stats(v, total) for k, v in times.items()}, "link_bytes_per_input_byte": link}
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
            f.write("stream_sentences.py --gib %s --reps %d --slice-mib %d\n%s\n" % (args.gib, args.reps, args.slice_mib, line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
