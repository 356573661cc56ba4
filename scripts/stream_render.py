#!/usr/bin/env python3
"""What a user of one long stream receives: the walk alone, the host writer's replay, and the device's rendering.

A single stream of --gib GiB from a cyclic reader (scripts/stream_throughput.py's: a 4 MiB period of German text) in
--slice-mib MiB slices at depth 3, tokenizer_de.matok, in a child process that never imports torch:

  leg a  dtk_stream_run with R_TOK_BYTE_BLK | R_EVENT_LIST | R_CSR | R_STATUS and an empty slice callback
  leg b  leg a replayed into the C++ TOKENS | SENTENCES writer (the replay of include/datok.hpp)
  leg c  rendering on (dtk_stream_set_render, mode 3), the same fields, the bytes counted and discarded in slice_fn
  leg p  a position mode replayed: dtk_stream_transduce in mode 15 (TOKENS | SENTENCES | TOKEN_POS | SENTENCE_POS) on the
         parent commit's build, where it feeds every slice to the C++ writer's closures
  leg e  the same mode rendered on the device (dtk_stream_set_position_render) and put together by dtk_stream_emit into a
         write_fn that counts the bytes and discards them

Legs alternate; median of --reps runs after one warm-up round, with min and max.  This build's dtk_stream_transduce
takes the rendered bytes in every mode, so legs b and p exist on a build of the parent commit only: --parent-tree names a
checkout of it with its library built, and legs a, b and p are run on that package in a second child of the same session.

Then the render kernels alone: the memset and the four kernels of dtk_launch_streamrender on one slice's arrays, 20
launches back to back between two HIP events on the batch's download stream, and beside them 20 copies of the bytes
they produce into page-locked memory ("kernels_one_slice").  The same for the position renderer in mode 15
("pos_kernels_one_slice"): the fill of the capacity bound, the eleven launches of dtk_launch_streampos, and the copy of
the bound with the trailer block, each timed on its own, with the bound and the real length per input byte.

usage: python scripts/stream_render.py [--gib 1] [--reps 3] [--slice-mib 16] [--parent-tree ab/parent]
                                       [--out profiles/stream_render.txt]
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


class _EvListArgs(C.Structure):   # DtkEvListArgs, dtk_internal.h
    _fields_ = [("bits", C.c_void_p), ("bit_words", C.c_uint32), ("n_docs", C.c_uint32), ("doc_off", C.c_void_p),
                ("n_bits", C.c_uint64), ("n_tiles", C.c_uint32), ("cap", C.c_uint32), ("tile_base", C.c_void_p),
                ("count", C.c_void_p), ("evl_off", C.c_void_p), ("evl_pos", C.c_void_p), ("evl_kind", C.c_void_p),
                ("evl_bit", C.c_void_p)]


class _RenderArgs(C.Structure):   # DtkStreamRenderArgs, dtk_internal.h
    _fields_ = [("bits", C.c_uint32), ("with_tail", C.c_uint32), ("text", C.c_void_p), ("text_len", C.c_uint32),
                ("sym_base", C.c_void_p), ("sym_lut", C.c_void_p), ("n_tok", C.c_uint64),
                ("tok_bstart", C.c_void_p), ("tok_bend", C.c_void_p), ("evl_pos", C.c_void_p), ("evl_kind", C.c_void_p),
                ("evl_count", C.c_void_p), ("evl_cap", C.c_uint32), ("doc_tail", C.c_void_p),
                ("tok_tiles", C.c_uint32), ("ent_tiles", C.c_uint32), ("tok_base", C.c_void_p), ("ent_base", C.c_void_p),
                ("ew", C.c_void_p), ("out", C.c_void_p), ("cap", C.c_uint64), ("out_len", C.c_void_p)]


def stats(seconds, total):
    return {"GBps_median": round(total / statistics.median(seconds) / 1e9, 3), "GBps_min": round(total / max(seconds) / 1e9, 3),
            "GBps_max": round(total / min(seconds) / 1e9, 3), "seconds": [round(s, 4) for s in seconds]}


def kernel_times(tok, S, launches=20):
    """Microseconds per rendering of one slice (memset + four kernels), and per copy of its bytes."""
    import numpy as np
    import datok_amd
    from datok_amd import host
    from stream_throughput import period_text
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    per = period_text(False)
    n = S + 8192
    text = np.frombuffer((per * (n // len(per) + 1))[:n], np.uint8)
    off = np.array([0, n], np.uint64)
    with datok_amd.Batch(n, 1) as b:
        b.set_input(text, off)
        b.run(tok, host.NO_RUNE_OFFSETS)
        t = b.totals()
        v = b.result_device()
        stream = C.c_void_p(L.dtk_batch_download_stream(b._h))
        rows = t["n_sent"] + t["n_texts"]
        L.dtk_evlist_tiles.argtypes, L.dtk_evlist_tiles.restype = [C.c_uint64, C.c_uint32], C.c_uint32
        L.dtk_launch_evlist.argtypes = [C.POINTER(_EvListArgs), C.c_void_p]
        L.dtk_streamrender_tiles.argtypes, L.dtk_streamrender_tiles.restype = [C.c_uint64], C.c_uint32
        L.dtk_launch_streamrender.argtypes = [C.POINTER(_RenderArgs), C.c_void_p]
        ev_tiles = L.dtk_evlist_tiles(n + 1, int(v.ev_words))
        tt, et = L.dtk_streamrender_tiles(t["n_tokens"]), L.dtk_streamrender_tiles(rows)
        cap = n + t["n_tokens"] + t["n_sent"] + t["n_texts"] + 2
        cap8 = (cap + 7) & ~7
        sizes = {"text": n, "doc_off": 16, "tile_base": 4 * max(ev_tiles, 1), "count": 4, "evl_off": 8, "evl_pos": 4 * rows,
                 "evl_kind": rows, "evl_bit": 4 * rows, "ws": 8 * (tt + et + rows + 1), "out": cap8 + 8}
        mem = {}
        for k, nb in sizes.items():
            mem[k] = C.c_void_p()
            ok(hip.hipMalloc(C.byref(mem[k]), C.c_size_t(max(nb, 16))))
        ok(hip.hipMemcpy(mem["text"], C.c_void_p(text.ctypes.data), C.c_size_t(n), 1))          # host to device
        ok(hip.hipMemcpy(mem["doc_off"], C.c_void_p(off.ctypes.data), C.c_size_t(16), 1))
        ea = _EvListArgs(v.ev_bits, int(v.ev_words), 1, mem["doc_off"], n + 1, ev_tiles, rows, mem["tile_base"],
                         mem["count"], mem["evl_off"], mem["evl_pos"], mem["evl_kind"], mem["evl_bit"])
        ok(L.dtk_launch_evlist(C.byref(ea), stream))
        ws = mem["ws"].value
        ra = _RenderArgs(3, 1, mem["text"], n, None, None, t["n_tokens"], v.tok_bstart, v.tok_bend, mem["evl_pos"],
                         mem["evl_kind"], mem["count"], rows, v.doc_tail, tt, et, ws, ws + 8 * tt, ws + 8 * (tt + et),
                         mem["out"], cap, mem["out"].value + cap8)
        pinned = C.c_void_p(L.dtk_pinned_alloc(cap8 + 8))
        assert pinned.value
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        out = {}
        for what in ("render", "copy"):
            us = []
            for rep in range(4):                      # (the first round is the warm-up)
                ok(hip.hipEventRecord(e0, stream))
                for _ in range(launches):
                    if what == "render":
                        ok(hip.hipMemsetAsync(mem["out"], 10, C.c_size_t(cap8), stream))
                        ok(L.dtk_launch_streamrender(C.byref(ra), stream))
                    else:
                        ok(hip.hipMemcpyAsync(pinned, mem["out"], C.c_size_t(cap8 + 8), 2, stream))      # device to host
                ok(hip.hipEventRecord(e1, stream))
                ok(hip.hipEventSynchronize(e1))
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
                if rep:
                    us.append(ms.value * 1e3 / launches)
            out[what + "_us"] = round(sorted(us)[len(us) // 2], 1)
        got = np.frombuffer((C.c_char * (cap8 + 8)).from_address(pinned.value), dtype=np.uint8)
        length = int(got[cap8:].view(np.uint64)[0])
        from oracle import oracle as O
        exp = O.Model(MODEL).transduce(text.tobytes(), 3)[0]
        out.update({"slice_bytes": n, "tokens": t["n_tokens"], "entries_bound": rows, "out_bytes": length, "copy_bytes": cap8 + 8,
                    "launches_per_sample": launches, "equals_the_oracles_bytes": bytes(got[:length]) == exp,
                    "what": "hipMemsetAsync + k_sr_sums + k_sr_scan + k_sr_entries + k_sr_copy on the download stream between "
                            "two HIP events; the copy: hipMemcpyAsync of the bound + the length word to page-locked memory"})
        L.dtk_pinned_free(pinned)
        for p in mem.values():
            ok(hip.hipFree(p))
        ok(hip.hipEventDestroy(e0))
        ok(hip.hipEventDestroy(e1))
    return out


class _PosArgs(C.Structure):      # DtkStreamPosArgs, dtk_internal.h (dtk_streampos_ws fills the workspace pointers)
    _fields_ = ([("bits", C.c_uint32), ("with_tail", C.c_uint32), ("is_matrix", C.c_uint32), ("first", C.c_uint32),
                 ("text", C.c_void_p), ("text_len", C.c_uint32), ("sym_base", C.c_void_p), ("sym_lut", C.c_void_p),
                 ("n_tok", C.c_uint64), ("tok_bstart", C.c_void_p), ("tok_bend", C.c_void_p), ("evl_pos", C.c_void_p),
                 ("evl_kind", C.c_void_p), ("evl_count", C.c_void_p), ("evl_cap", C.c_uint32), ("doc_tail", C.c_void_p),
                 ("tok_tiles", C.c_uint32), ("ent_tiles", C.c_uint32), ("carry_in", C.c_void_p), ("carry_out", C.c_void_p)]
                + [(k, C.c_void_p) for k in ("hdr", "ent_base", "cnt", "ew", "ent_pre", "te_idx", "seg_pos", "seg_sent", "seg_pw0",
                                             "seg_sw0", "tile_sum", "tile_in", "tile_flag", "w_base", "rstart", "rend", "tok_v",
                                             "tok_len", "tok_meta", "tok_seg", "w_in")]
                + [("out", C.c_void_p), ("cap", C.c_uint64), ("trailer", C.c_void_p)])


def pos_kernel_times(tok, S, launches=10, digits=8):
    """Microseconds, for one slice in mode 15: the fill of the capacity bound, the position renderer's launches, and the
    copy of the bound and the trailer block; the bound (dtk_results.cpp, render_slice_pos, with integers of up to `digits`
    bytes: what a stream of 16 MiB slices at depth 3 is sized for) and the real length."""
    import numpy as np
    import datok_amd
    from datok_amd import host
    from stream_throughput import period_text
    L = datok_amd.lib()
    hip = C.CDLL("libamdhip64.so")

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    per = period_text(False)
    n = S + 8192
    text = np.frombuffer((per * (n // len(per) + 1))[:n], np.uint8)
    off = np.array([0, n], np.uint64)
    TRAILER = 96
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
        L.dtk_streampos_ws.argtypes, L.dtk_streampos_ws.restype = [C.POINTER(_PosArgs), C.c_void_p], C.c_uint64
        L.dtk_launch_streampos.argtypes = [C.POINTER(_PosArgs), C.c_void_p]
        ev_tiles = L.dtk_evlist_tiles(n + 1, int(v.ev_words))
        calls = 3 * rows + 2
        ints = 2 * nt + min(nt, calls + 1) + 2 * rows + 1
        cap = n + nt + calls + ints * (digits + 1) + 2 * (rows + 2)
        cap8 = (cap + 7) & ~7
        pa = _PosArgs(bits=15, with_tail=1, is_matrix=1, first=0, text_len=n, n_tok=nt, tok_bstart=v.tok_bstart,
                      tok_bend=v.tok_bend, evl_cap=rows, doc_tail=v.doc_tail, tok_tiles=L.dtk_streamrender_tiles(nt),
                      ent_tiles=L.dtk_streamrender_tiles(rows), cap=cap)
        words = L.dtk_streampos_ws(C.byref(pa), None)
        sizes = {"text": n, "doc_off": 16, "tile_base": 4 * max(ev_tiles, 1), "count": 4, "evl_off": 8, "evl_pos": 4 * rows,
                 "evl_kind": rows, "evl_bit": 4 * rows, "ws": 8 * words, "out": cap8 + TRAILER, "carry": 48}
        mem = {}
        for k, nb in sizes.items():
            mem[k] = C.c_void_p()
            ok(hip.hipMalloc(C.byref(mem[k]), C.c_size_t(max(nb, 16))))
        ok(hip.hipMemcpy(mem["text"], C.c_void_p(text.ctypes.data), C.c_size_t(n), 1))          # host to device
        ok(hip.hipMemcpy(mem["doc_off"], C.c_void_p(off.ctypes.data), C.c_size_t(16), 1))
        carry0 = np.array([0, 0, 1, 1, 0, 0], np.uint32)       # {posC 0 (64 bits), sentB, init, pos / sent empty}
        ok(hip.hipMemcpy(mem["carry"], C.c_void_p(carry0.ctypes.data), C.c_size_t(24), 1))
        ea = _EvListArgs(v.ev_bits, int(v.ev_words), 1, mem["doc_off"], n + 1, ev_tiles, rows, mem["tile_base"],
                         mem["count"], mem["evl_off"], mem["evl_pos"], mem["evl_kind"], mem["evl_bit"])
        ok(L.dtk_launch_evlist(C.byref(ea), stream))
        pa.text, pa.evl_pos, pa.evl_kind, pa.evl_count = mem["text"], mem["evl_pos"], mem["evl_kind"], mem["count"]
        pa.carry_in, pa.carry_out = mem["carry"].value, mem["carry"].value + 24
        assert L.dtk_streampos_ws(C.byref(pa), mem["ws"]) == words
        pa.out, pa.trailer = mem["out"], mem["out"].value + cap8
        pinned = C.c_void_p(L.dtk_pinned_alloc(cap8 + TRAILER))
        assert pinned.value
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        out = {}
        for what in ("fill", "kernels", "copy"):
            us = []
            for rep in range(4):                      # (the first round is the warm-up)
                ok(hip.hipEventRecord(e0, stream))
                for _ in range(launches):
                    if what == "fill":
                        ok(hip.hipMemsetAsync(mem["out"], 10, C.c_size_t(cap8), stream))
                    elif what == "kernels":
                        ok(L.dtk_launch_streampos(C.byref(pa), stream))
                    else:
                        ok(hip.hipMemcpyAsync(pinned, mem["out"], C.c_size_t(cap8 + TRAILER), 2, stream))      # device to host
                ok(hip.hipEventRecord(e1, stream))
                ok(hip.hipEventSynchronize(e1))
                ms = C.c_float()
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
                if rep:
                    us.append(ms.value * 1e3 / launches)
            out[what + "_us"] = round(sorted(us)[len(us) // 2], 1)
        # one clean rendering for the comparison: fill, kernels, copy
        ok(hip.hipMemsetAsync(mem["out"], 10, C.c_size_t(cap8), stream))
        ok(L.dtk_launch_streampos(C.byref(pa), stream))
        ok(hip.hipMemcpyAsync(pinned, mem["out"], C.c_size_t(cap8 + TRAILER), 2, stream))
        ok(hip.hipStreamSynchronize(stream))
        got = np.frombuffer((C.c_char * (cap8 + TRAILER)).from_address(pinned.value), dtype=np.uint8)
        tr = got[cap8:cap8 + 40].view(np.uint64)
        length = int(tr[0])
        from oracle import oracle as O
        exp = O.Model(MODEL).transduce(text.tobytes(), 15)[0]
        out.update({"mode": 15, "slice_bytes": n, "tokens": nt, "entries_bound": rows, "digits_bound": digits, "out_bytes": length,
                    "open_bytes": int(tr[1]) + int(tr[2]), "copy_bytes": cap8 + TRAILER,
                    "copy_bytes_per_input_byte": round((cap8 + TRAILER) / n, 3), "out_bytes_per_input_byte": round(length / n, 3),
                    "launches_per_sample": launches, "equals_the_oracles_bytes": length <= cap and bytes(got[:length]) == exp,
                    "what": "each on its own between two HIP events on the download stream: hipMemsetAsync of the bound; "
                            "dtk_launch_streampos (k_sp_ent_count x2, k_sp_scan x4, k_sp_tok_runes, k_sp_tok_weights, "
                            "k_sp_ent_weights, k_sp_ent_offsets, k_sp_write); hipMemcpyAsync of the bound + the trailer block "
                            "to page-locked memory"})
        L.dtk_pinned_free(pinned)
        for p in mem.values():
            ok(hip.hipFree(p))
        ok(hip.hipEventDestroy(e0))
        ok(hip.hipEventDestroy(e1))
    return out


def child(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
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
    parent = "b" in args.legs
    if args.kernels_only:
        print(json.dumps({"build": "this", "slice_bytes": S, "kernels_one_slice": kernel_times(tok, S),
                          "pos_kernels_one_slice": pos_kernel_times(tok, S)}))
        return
    st = host.Stream(S, depth=3)
    st.set_result_fields(fields)
    times = {k: [] for k in args.legs}
    counts = {}
    for rep in range(args.reps + 1):                # (the first round warms up and is dropped)
        for leg in args.legs:
            status = C.c_uint32(0)
            if leg in "ace":
                if not parent:
                    st.set_render(3 if leg == "c" else None)
                    st.set_position_render(15 if leg == "e" else None)
                n = [0, 0]

                def discard(_u, _p, nb):
                    n[1] += nb
                    return 0
                wr = _lib.WRITE_FN(discard) if leg == "e" else None

                def on_slice(_u, p):
                    s = p.contents
                    n[0] += int(C.cast(s.view.tok_off, C.POINTER(C.c_uint64))[1])
                    if leg == "c":
                        n[1] += int(s.out_len)
                    if leg == "e":
                        return L.dtk_stream_emit(st._h, wr, None)
                    return 0
                t0 = time.perf_counter()
                rc = L.dtk_stream_run(st._h, tok._h, _lib.READ_FN(Cyclic(per, total).fn()), None, 0,
                                      _lib.STREAM_SLICE_FN(on_slice), None, C.byref(status))
                t1 = time.perf_counter()
                counts[leg + "_tokens"] = n[0]
                if leg in "ce":
                    counts[leg + "_bytes"] = n[1]
            else:
                o, nb = C.c_void_p(), C.c_size_t()
                t0 = time.perf_counter()
                rc = L.dtk_stream_transduce(st._h, tok._h, _lib.READ_FN(Cyclic(per, total).fn()), None, 3 if leg == "b" else 15,
                                            C.byref(o), C.byref(nb), C.byref(status))
                t1 = time.perf_counter()
                counts[leg + "_bytes"] = nb.value
                L.dtk_free(o)
            assert rc == 0 and status.value == 0, (leg, rc, status.value)
            if rep:
                times[leg].append(t1 - t0)
    out = {"build": "parent" if parent else "this", "lib": _lib.LIB_PATH, "bytes": total, "slice_bytes": S, "reps": args.reps,
           "legs": {k: stats(v, total) for k, v in times.items()}, **counts}
    st.close()
    if not parent:
        out["kernels_one_slice"] = kernel_times(tok, S)
        out["pos_kernels_one_slice"] = pos_kernel_times(tok, S)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slice-mib", type=int, default=16)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, built: legs a, b and p run on it")
    ap.add_argument("--tree", default=None, help="(internal) the child imports datok_amd from here")
    ap.add_argument("--out", default=None)
    ap.add_argument("--legs", default="ace", help="(internal) the child's legs")
    ap.add_argument("--kernels-only", action="store_true", help="only the two renderers' kernels on one slice, no legs")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    if args.child or args.kernels_only:
        return child(args)
    lines = []
    for legs, tree in (("ace", None), ("abp", args.parent_tree)):
        if legs == "abp" and not tree:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--legs", legs, "--gib", str(args.gib), "--reps", str(args.reps),
               "--slice-mib", str(args.slice_mib)]
        env = {k: v for k, v in os.environ.items() if not k.startswith("DATOK_")}
        if tree:
            cmd += ["--tree", tree]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=1500)
        line = r.stdout.decode().strip().split("\n")[-1] if r.stdout else ""
        print(line, flush=True)
        if r.returncode != 0:
            return r.returncode
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("stream_render.py --gib %s --reps %d --slice-mib %d\n%s\n" % (args.gib, args.reps, args.slice_mib, "\n".join(lines)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
