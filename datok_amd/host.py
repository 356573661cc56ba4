"""Host-side mirror of Datok's Go API over the C-ABI (no compute here)."""
import ctypes as C
import io
import sys

import numpy as np

from . import _lib
from ._lib import ModelInfo, RenderView, ResultView, SentenceView, Totals, check, lib

# token_writer.go:17-25
TOKENS, SENTENCES, TOKEN_POS, SENTENCE_POS, NEWLINE_AFTER_EOT = 1, 2, 4, 8, 16
SIMPLE = TOKENS | SENTENCES
# dtk_batch_run only (datok_gpu.h): no renderer bookkeeping / only one kind of token offsets
OFFSETS_ONLY, NO_BYTE_OFFSETS, NO_RUNE_OFFSETS = 256, 512, 1024

# calls at one cursor position, in the order they fire (flag byte of event_bytes(); datok_gpu.h DTK_EVB_* / DTK_TAIL_*)
EV_S_EOT, EV_E_EOT, EV_TOK_END, EV_S_EPS, EV_S_EOF, EV_E_EOF = 1, 2, 4, 8, 32, 64
EVB_END, EVB_START, EVB_SEPS, EVB_TEOT, EVB_SEOT = 0, 1, 2, 3, 4
# bits of an event list entry's kind (datok_gpu.h DTK_EVL_*), in the order the calls fire around a Token at one cursor
EVL_SEOT, EVL_TEOT, EVL_SEPS = 1, 2, 4


# ------------------------------------------------------------------ UTF-8 (Go)
def _decode_runes(b: bytes):
    """Go's rune iteration: invalid bytes become U+FFFD of width 1."""
    if isinstance(b, bytes) and b.isascii():
        return list(b)
    out, i, n = [], 0, len(b)
    while i < n:
        b0 = b[i]
        r, w = 0xFFFD, 1
        if b0 < 0x80:
            r = b0
        elif 0xC2 <= b0 < 0xE0:
            if i + 1 < n and (b[i + 1] & 0xC0) == 0x80:
                r, w = ((b0 & 0x1F) << 6) | (b[i + 1] & 0x3F), 2
        elif 0xE0 <= b0 < 0xF0:
            lo, hi = (0xA0 if b0 == 0xE0 else 0x80), (0x9F if b0 == 0xED else 0xBF)
            if i + 2 < n and lo <= b[i + 1] <= hi and (b[i + 2] & 0xC0) == 0x80:
                r, w = ((b0 & 0x0F) << 12) | ((b[i + 1] & 0x3F) << 6) | (b[i + 2] & 0x3F), 3
        elif 0xF0 <= b0 <= 0xF4:
            lo, hi = (0x90 if b0 == 0xF0 else 0x80), (0x8F if b0 == 0xF4 else 0xBF)
            if (i + 3 < n and lo <= b[i + 1] <= hi and (b[i + 2] & 0xC0) == 0x80
                    and (b[i + 3] & 0xC0) == 0x80):
                r, w = (((b0 & 0x07) << 18) | ((b[i + 1] & 0x3F) << 12)
                        | ((b[i + 2] & 0x3F) << 6) | (b[i + 3] & 0x3F)), 4
        out.append(r)
        i += w
    return out


def _runes_to_bytes(runes):
    return "".join(chr(r) if not (0xD800 <= r <= 0xDFFF or r > 0x10FFFF) else "�"
                   for r in runes).encode("utf-8")


# ----------------------------------------------------------------- TokenWriter
class TokenWriter:
    """token_writer.go:27-33: four closures."""
    __slots__ = ("SentenceEnd", "TextEnd", "Flush", "Token")


def new_token_writer(w, flags) -> TokenWriter:
    """token_writer.go:36-175 NewTokenWriter. `w` is a binary file-like object."""
    st = {"posC": 0, "pos": [], "sentB": True, "sent": [], "init": True}
    out = bytearray()
    tw = TokenWriter()

    def flush():
        if out:
            w.write(bytes(out))
            out.clear()
        if hasattr(w, "flush"):
            w.flush()

    def surface(offset, buf):
        out.extend(_runes_to_bytes(buf[offset:]))
        out.append(10)

    if flags & (TOKEN_POS | SENTENCE_POS):
        def token(offset, buf):
            if st["posC"] == 0 and flags & NEWLINE_AFTER_EOT and buf and buf[0] == 10 and not st["init"]:
                st["posC"] -= 1
            st["init"] = False
            st["posC"] += offset
            st["pos"].append(st["posC"])
            if st["sentB"]:
                st["sentB"] = False
                st["sent"].append(st["posC"])
            st["posC"] += len(buf) - offset
            st["pos"].append(st["posC"])
            if flags & TOKENS:
                surface(offset, buf)
    elif flags & TOKENS:
        token = surface
    else:
        def token(offset, buf):
            pass
    tw.Token = token

    if flags & SENTENCE_POS:
        def sentence_end(_):
            st["sent"].append(st["pos"][-1])     # Go panics on an empty pos
            st["sentB"] = True
            if flags & SENTENCES:
                out.append(10)
    elif flags & SENTENCES:
        def sentence_end(_):
            out.append(10)
            flush()
    else:
        def sentence_end(_):
            pass
    tw.SentenceEnd = sentence_end

    if flags & (TOKEN_POS | SENTENCE_POS):
        def text_end(_):
            if flags & TOKEN_POS:
                out.extend(" ".join(map(str, st["pos"])).encode() if st["pos"] else b"")
                st["pos"][0]                      # Go: pos[0] panics on an empty text
                out.append(10)
            if flags & SENTENCE_POS:
                st["sent"][0]
                out.extend(" ".join(map(str, st["sent"])).encode())
                out.append(10)
                st["sent"] = []
                st["sentB"] = True
            flush()
            st["posC"] = 0
            st["pos"] = []
    else:
        def text_end(_):
            out.append(10)
            flush()
    tw.TextEnd = text_end
    tw.Flush = flush
    return tw


def event_bytes(ev_bits, doc_off_d, d, n, tail):
    """One flag byte per cursor position 0..n of document d (EV_* bits, bit order = call order) from the event
    bitmaps of a host dtk_result_view (ev_bits: uint32[kinds, words]) and the document's tail word."""
    g0 = int(doc_off_d) + int(d)
    w0, w1 = g0 >> 5, (g0 + n + 32) >> 5
    out = np.zeros(n + 1, dtype=np.uint8)
    for kind, flag in ((EVB_SEOT, EV_S_EOT), (EVB_TEOT, EV_E_EOT), (EVB_END, EV_TOK_END), (EVB_SEPS, EV_S_EPS)):
        words = np.ascontiguousarray(ev_bits[kind, w0:w1 + 1])
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[g0 - 32 * w0: g0 - 32 * w0 + n + 1]
        out |= bits * np.uint8(flag)
    tail = int(tail)
    if tail & 3:
        out[min(tail >> 2, n)] |= (EV_S_EOF if tail & 1 else 0) | (EV_E_EOF if tail & 2 else 0)
    return out


def replay(is_matrix, text: bytes, events, tok_bstart, tw: TokenWriter):
    """Feeds one document's events (event_bytes()) to the closures in reference call order.

    Int arguments as upstream: the matrix passes buffc (matrix.go:575,597,600,684,691);
    the double array 0, except SentenceEnd(buffc) at EOT (datok.go:1015,1023,1026)."""
    n = len(text)
    B = k = 0
    nz = np.flatnonzero(np.asarray(events[:n + 1]))
    for p in nz.tolist():
        e = int(events[p])
        def buffc():
            return len(_decode_runes(text[B:p]))
        if e & EV_S_EOT:
            tw.SentenceEnd(buffc())
        if e & EV_E_EOT:
            tw.TextEnd(buffc() if is_matrix else 0)
            if is_matrix:
                B = p
        if e & EV_TOK_END:
            start = int(tok_bstart[k])
            k += 1
            buf = _decode_runes(text[B:p])
            tw.Token(len(_decode_runes(text[B:start])), buf)
            B = p
        if e & EV_S_EPS:
            tw.SentenceEnd(buffc() if is_matrix else 0)
        if e & EV_S_EOF:
            tw.SentenceEnd(buffc() if is_matrix else 0)
        if e & EV_E_EOF:
            tw.TextEnd(buffc() if is_matrix else 0)


def replay_list(is_matrix, text: bytes, evl_pos, evl_kind, tail, tok_bstart, tok_bend, tw: TokenWriter):
    """The same from one document's event list (Batch.R_EVENT_LIST: evl_pos / evl_kind, datok_gpu.h) instead of its
    event bytes: the tokens (cursor tok_bend[k], first byte tok_bstart[k]) and the entries are merged by position; at
    one cursor SEOT, TEOT, the Token ending there, SEPS; the tail word's SentenceEnd / TextEnd come last.  O(tokens +
    entries).  The int arguments are replay()'s."""
    n = len(text)
    B = k = j = 0
    nt, ne = len(tok_bend), len(evl_pos)
    while k < nt or j < ne:
        pt = int(tok_bend[k]) if k < nt else n + 1
        pe = int(evl_pos[j]) if j < ne else n + 1
        p = min(pt, pe)
        e = 0
        if pe == p:
            e = int(evl_kind[j])
            j += 1
        def buffc():
            return len(_decode_runes(text[B:p]))
        if e & EVL_SEOT:
            tw.SentenceEnd(buffc())
        if e & EVL_TEOT:
            tw.TextEnd(buffc() if is_matrix else 0)
            if is_matrix:
                B = p
        if pt == p:
            start = int(tok_bstart[k])
            k += 1
            tw.Token(len(_decode_runes(text[B:start])), _decode_runes(text[B:p]))
            B = p
        if e & EVL_SEPS:
            tw.SentenceEnd(buffc() if is_matrix else 0)
    tail = int(tail)
    p = min(tail >> 2, n)
    if tail & 1:
        tw.SentenceEnd(len(_decode_runes(text[B:p])) if is_matrix else 0)
    if tail & 2:
        tw.TextEnd(len(_decode_runes(text[B:p])) if is_matrix else 0)


class SliceView:
    """One slice of a stream (dtk_stream_slice, datok_gpu.h) in host arrays.  All positions are relative to the
    slice's window `text`, whose byte 0 is stream byte `base`: the slice's calls begin with the reference's window
    start (buffer[0]) at `first` and end at `cut`; `tail` (doc_tail) counts on the `last` slice only.  `out`: the bytes
    a stock writer writes for the slice's calls as the device rendered them (Stream.set_render), else None.
    In a position mode (Stream.set_position_render) `out` lacks the integers of a text that other slices share:
    splice_pos / splice_sent (None: no such place) are the offsets where the integers held from earlier slices belong,
    open_pos / open_sent the integers of the text still open at the cut, carry_in / carry_out the writer's state
    (posC, sentB, init, pos non-empty, sent non-empty) in front of and behind the slice, and `written` the slice's
    final bytes (dtk_stream_emit).  (This view is the tests' and scripts' mirror: with position rendering on it runs
    dtk_stream_emit for every slice and keeps a second copy of the bytes in `written`; a caller that wants the bytes
    once calls dtk_stream_emit from its own slice callback, as scripts/stream_render.py does.)
    With Stream.set_offsets the slice brings what a writer with TOKEN_POS | SENTENCE_POS collects during its calls, as
    arrays (dtk_stream_offsets; None when it is off): r_tok_rstart / r_tok_rend (int64, decoded from whichever form
    came; r_blocked says whether that was the blocked one, r_rblk / r_rblk_head are its words and heads), r_sent (int64),
    r_text_tok_end / r_text_sent_end (tokens / sent ints of THIS slice in front of each TextEnd), r_carry_in /
    r_carry_out (the writer's state as above).
    With Stream.set_sentences the slice brings the sentences its calls close, as rows (dtk_stream_sentences; None when
    it is off): s_tok_end (uint32: tokens of THIS slice up to and including the row's last), s_bstart / s_bend (uint64,
    stream byte offsets), s_rstart / s_rend (int64, the writer's rune offsets), s_text_sen_end (rows of THIS slice closed
    in front of each TextEnd), s_carry_in / s_carry_out (the row open at the cut: (open, bstart, bend, rstart, rend)).
    With Stream.set_vocab the slice brings tok_id (np.int32, one per token of the slice; None with ids_home=False) and
    n_unknown (dtk_stream_token_ids; both None when it is off).
    With Stream.set_wordpiece the slice brings its tokens' pieces (dtk_stream_pieces; all None when it is off): piece_off
    (np.uint64, tokens of THIS slice + 1, from 0), piece_id (np.int32), piece_bend (np.uint32, relative to the slice's
    window like tok_bend) -- the three None with pieces_home=False -- and n_pieces, n_piece_unknown."""
    __slots__ = ("base", "first", "cut", "text", "last", "status", "tok_bstart", "tok_bend", "evl_pos", "evl_kind", "tail",
                 "out", "splice_pos", "splice_sent", "open_pos", "open_sent", "carry_in", "carry_out", "written",
                 "r_tok_rstart", "r_tok_rend", "r_blocked", "r_rblk", "r_rblk_head", "r_sent", "r_text_tok_end",
                 "r_text_sent_end", "r_carry_in", "r_carry_out",
                 "s_tok_end", "s_bstart", "s_bend", "s_rstart", "s_rend", "s_text_sen_end", "s_carry_in", "s_carry_out",
                 "tok_id", "n_unknown", "piece_off", "piece_id", "piece_bend", "n_pieces", "n_piece_unknown")
    _NONE = ("out", "splice_pos", "splice_sent", "open_pos", "open_sent", "carry_in", "carry_out", "written",
             "r_tok_rstart", "r_tok_rend", "r_blocked", "r_rblk", "r_rblk_head", "r_sent", "r_text_tok_end",
             "r_text_sent_end", "r_carry_in", "r_carry_out",
             "s_tok_end", "s_bstart", "s_bend", "s_rstart", "s_rend", "s_text_sen_end", "s_carry_in", "s_carry_out",
             "tok_id", "n_unknown", "piece_off", "piece_id", "piece_bend", "n_pieces", "n_piece_unknown")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k, None if k in self._NONE else 0))


def slice_calls(is_matrix, sl: SliceView):
    """The reference's calls of one slice, in its order: ('T', B, start, end) for Token(offset, buf) with buf =
    text[B:end] and buf[offset:] = text[start:end]; ('S', B, p) / ('E', B, p) for SentenceEnd / TextEnd at cursor p
    (B: the window start then).  replay_list()'s merge, with the window start beginning at sl.first instead of 0."""
    n = len(sl.text)
    B = int(sl.first)
    k = j = 0
    nt, ne = len(sl.tok_bend), len(sl.evl_pos)
    while k < nt or j < ne:
        pt = int(sl.tok_bend[k]) if k < nt else n + 1
        pe = int(sl.evl_pos[j]) if j < ne else n + 1
        p = min(pt, pe)
        e = 0
        if pe == p:
            e = int(sl.evl_kind[j])
            j += 1
        if e & EVL_SEOT:
            yield ("S", B, p, True)
        if e & EVL_TEOT:
            yield ("E", B, p, is_matrix)
            if is_matrix:
                B = p
        if pt == p:
            yield ("T", B, int(sl.tok_bstart[k]), p)
            k += 1
            B = p
        if e & EVL_SEPS:
            yield ("S", B, p, is_matrix)
    if sl.last:
        tail = int(sl.tail)
        p = min(tail >> 2, n)
        if tail & 1:
            yield ("S", B, p, is_matrix)
        if tail & 2:
            yield ("E", B, p, is_matrix)


def replay_slice(is_matrix, sl: SliceView, tw: TokenWriter):
    """Feeds one slice of a stream to the closures of the stream's ONE writer (posC, sentB and init of NewTokenWriter
    run across cuts, token_writer.go:38-42).  The int arguments are replay()'s."""
    text = sl.text
    for c in slice_calls(is_matrix, sl):
        if c[0] == "T":
            _, B, start, end = c
            tw.Token(len(_decode_runes(text[B:start])), _decode_runes(text[B:end]))
        else:
            kind, B, p, counted = c
            arg = len(_decode_runes(text[B:p])) if counted else 0
            (tw.SentenceEnd if kind == "S" else tw.TextEnd)(arg)


def replay_calls(text: bytes, calls, tw: TokenWriter):
    """Feeds the call list of a document walked by the exact pass (dtk_result_view.calls: rows of
    (kind, a, b, c)) to the closures: kind 0 Token(offset, buf) with buf = runes of text[a:c] and offset =
    runes of text[a:b]; kind 1 SentenceEnd(a); kind 2 TextEnd(a)."""
    for kind, a, b, c in calls:
        if kind == 0:
            tw.Token(len(_decode_runes(text[a:b])), _decode_runes(text[a:c]))
        elif kind == 1:
            tw.SentenceEnd(a)
        else:
            tw.TextEnd(a)


def _exact_calls(v, arr):
    """dict doc id -> list of (kind, a, b, c) from a host dtk_result_view."""
    n = int(v.n_exact)
    if n == 0:
        return {}
    ids = arr(v.exact_doc, n, np.uint32)
    off = arr(v.exact_off, n + 1, np.uint64)
    calls = arr(v.calls, int(off[-1]) * 4, np.int32).reshape(-1, 4)
    return {int(ids[i]): [(int(k) & 0xFFFFFFFF, int(a), int(b) & 0xFFFFFFFF, int(c) & 0xFFFFFFFF)
                          for k, a, b, c in calls[int(off[i]):int(off[i + 1])]] for i in range(n)}


# statuses on which the reference cannot finish a document whatever the writer does (matrix.go:365,406 index
# panic; a walk that left the table; the lookup cap; an internal check): TransduceTokenWriter returns false
_FATAL = _lib.ST_WINDOW_OVERFLOW | _lib.ST_BAD_MODEL | _lib.ST_STEP_LIMIT | _lib.ST_INTERNAL | _lib.ST_IRREGULAR


# ------------------------------------------------------------------- Tokenizer
class Tokenizer:
    """fomafile.go:29-33 Tokenizer, backed by a device-resident model."""

    def __init__(self, handle):
        self._h = handle
        info = ModelInfo()
        check(lib().dtk_model_get_info(self._h, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in ModelInfo._fields_}
        self.last_status = 0

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_model_free(h)

    def type(self) -> str:
        """matrix.go:102 / datok.go:252"""
        return lib().dtk_model_type(self._h).decode()

    def transduce(self, r, w) -> bool:
        """matrix.go:340-342: TransduceTokenWriter(r, NewTokenWriter(w, SIMPLE))."""
        return self.transduce_token_writer(r, new_token_writer(w, SIMPLE))

    def transduce_token_writer(self, r, tw: TokenWriter, slice_bytes=None) -> bool:
        """matrix.go:348-698 / datok.go:781-1135. One reader = one document.

        slice_bytes: the reader is a stream of unknown (any) length -- it is read and walked in slices of that many
        bytes with bounded memory (Stream, dtk_stream_run) and replayed slice by slice into the one writer."""
        if slice_bytes is not None:
            is_matrix = self.type() == "MATOK"
            try:
                with Stream(slice_bytes) as st:
                    self.last_status = st.run(self, r, on_slice=lambda sl: replay_slice(is_matrix, sl, tw))
            except _lib.DatokGpuError as e:        # the reference returns false
                print("datok_amd:", e, file=sys.stderr)
                return False
            tw.Flush()
            return not (self.last_status & _FATAL)
        text = r.read() if hasattr(r, "read") else bytes(r)
        if isinstance(text, str):
            text = text.encode("utf-8")
        v = ResultView()   # dtk_transduce_result: the library's per-thread batch, host pointers
        rc = lib().dtk_transduce_result(self._h, text, len(text), 0, C.byref(v))
        if rc != _lib.OK:                      # the reference returns false
            print("datok_amd:", _lib.DatokGpuError(rc, "dtk_transduce_result"), file=sys.stderr)
            return False
        n_ev = len(text) + 1
        ntok = int(np.frombuffer((C.c_char * 16).from_address(v.tok_off), dtype=np.uint64)[1])

        def arr(ptr, n, dt):
            return np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt) if n else np.zeros(0, dt)
        self.last_status = int(arr(v.status, 1, np.uint32)[0])
        exact = _exact_calls(v, arr)
        if 0 in exact:                          # walked by the exact pass: its calls are listed in order
            replay_calls(text, exact[0], tw)
        else:
            bits = arr(v.ev_bits, 5 * int(v.ev_words), np.uint32).reshape(5, -1)
            events = event_bytes(bits, 0, 0, len(text), arr(v.doc_tail, 1, np.uint32)[0])
            replay(self.type() == "MATOK", text, events, arr(v.tok_bstart, ntok, np.uint32), tw)
        tw.Flush()                              # `defer w.Flush()`, matrix.go:374
        return not (self.last_status & _FATAL)

    def transduce_bytes(self, text: bytes, flags=SIMPLE, replay=False):
        """dtk_transduce(): walked and rendered on the device; replay=True: dtk_transduce_replay(), the
        event bytes replayed into the C++ host mirror of NewTokenWriter. Returns (output, status)."""
        out, n, st = C.c_void_p(), C.c_size_t(), C.c_uint32()
        fn = lib().dtk_transduce_replay if replay else lib().dtk_transduce
        check(fn(self._h, text, len(text), flags, C.byref(out), C.byref(n), C.byref(st)))
        try:
            return C.string_at(out, n.value), st.value
        finally:
            lib().dtk_free(out)


def load_tokenizer_file(path):
    """fomafile.go:452-484: returns None (and logs) on any failure."""
    h = C.c_void_p()
    rc = lib().dtk_model_load(str(path).encode(), C.byref(h))
    if rc != _lib.OK:
        if rc in (_lib.E_NO_DEVICE, _lib.E_HIP):
            raise _lib.DatokGpuError(rc, "load_tokenizer_file")   # environment, not the file
        print("datok_amd: %s: %s" % (path, lib().dtk_strerror(rc).decode()), file=sys.stderr)
        return None
    return Tokenizer(h)


# ----------------------------------------------------------------------- Batch
def event_bit(doc_off_d, d):
    """DTK_EVENT_BIT: bit of position 0 of document d in the event bitmaps."""
    return int(doc_off_d) + int(d)


def unpack_blocked(words, heads, first=0, last=None):
    """(start, end) as int32 arrays from the blocked form of a pair of offset arrays (dtk_off_block, datok_gpu.h;
    what dtk_blk_start / dtk_blk_end give token by token).  words: uint32[n]; heads: int32[ceil(n / 64), 4] with
    the columns base0, base1, brk, reserved.  first / last: only the tokens [first, last) of the batch."""
    words = np.asarray(words, dtype=np.uint32)
    heads = np.asarray(heads).view(np.int32).reshape(-1, 4)
    i = np.arange(int(first), len(words) if last is None else int(last), dtype=np.int64)
    h = heads[i >> 6]
    base = np.where((i & 63) < h[:, 2], h[:, 0], h[:, 1]).astype(np.int32)
    w = words[i]
    return base + (w & np.uint32(0xFFFF)).astype(np.int32), base + (w >> np.uint32(16)).astype(np.int32)


HEAD64 = np.dtype([("base0", np.int64), ("base1", np.int64), ("brk", np.uint32), ("reserved", np.uint32)])  # dtk_off_block64


def unpack_blocked64(words, heads):
    """(start, end) as int64 arrays from the blocked form of a stream slice's rune offsets (dtk_off_block64, datok_gpu.h;
    what dtk_blk64_start / dtk_blk64_end give token by token).  words: uint32[n]; heads: HEAD64[ceil(n / 64)]."""
    words = np.asarray(words, dtype=np.uint32)
    heads = np.asarray(heads).view(HEAD64).reshape(-1)
    i = np.arange(len(words), dtype=np.int64)
    h = heads[i >> 6]
    base = np.where((i & 63) < h["brk"], h["base0"], h["base1"]).astype(np.int64)
    return base + (words & np.uint32(0xFFFF)).astype(np.int64), base + (words >> np.uint32(16)).astype(np.int64)


class BatchResult:
    """Host copy of dtk_result_view (CSR over documents)."""
    __slots__ = ("tok_off", "sent_off", "text_off", "tok_rstart", "tok_rend", "tok_bstart",
                 "tok_bend", "sent", "text_tok_end", "text_sent_end", "status", "ev_bits", "doc_tail", "doc_off", "exact",
                 "tok_r16", "tok_rblk", "tok_rblk_head", "tok_bblk", "tok_bblk_head", "evl_off", "evl_pos", "evl_kind")

    def events(self, d):
        """Flag byte per cursor position of document d (event_bytes()), for replays."""
        n = int(self.doc_off[d + 1]) - int(self.doc_off[d])
        return event_bytes(self.ev_bits, self.doc_off[d], d, n, self.doc_tail[d])

    def doc(self, d):
        """The rows of document d (arrays the run did not write or the caller did not select are empty)."""
        a, b = int(self.tok_off[d]), int(self.tok_off[d + 1])
        s0, s1 = int(self.sent_off[d]), int(self.sent_off[d + 1])
        t0, t1 = int(self.text_off[d]), int(self.text_off[d + 1])
        rs, re = self.tok_rstart[a:b], self.tok_rend[a:b]
        if len(self.tok_r16) and not len(self.tok_rstart):  # (R_TOK_RUNE16: int16 pairs {start, end})
            rs, re = self.tok_r16[a:b, 0].astype(np.int32), self.tok_r16[a:b, 1].astype(np.int32)
        elif len(self.tok_rblk) and not len(self.tok_rstart):  # (R_TOK_RUNE_BLK: 16-bit blocks)
            rs, re = unpack_blocked(self.tok_rblk, self.tok_rblk_head, a, b)
        bs, be = self.tok_bstart[a:b], self.tok_bend[a:b]
        if len(self.tok_bblk) and not len(self.tok_bstart):    # (R_TOK_BYTE_BLK)
            bs, be = (x.astype(np.uint32) for x in unpack_blocked(self.tok_bblk, self.tok_bblk_head, a, b))
        e0, e1 = (int(self.evl_off[d]), int(self.evl_off[d + 1])) if len(self.evl_off) else (0, 0)   # (R_EVENT_LIST)
        return dict(tok_rstart=rs, tok_rend=re,
                    tok_bstart=bs, tok_bend=be, evl_pos=self.evl_pos[e0:e1], evl_kind=self.evl_kind[e0:e1],
                    sent=self.sent[s0:s1], text_tok_end=self.text_tok_end[t0:t1],
                    text_sent_end=self.text_sent_end[t0:t1], status=int(self.status[d]))


class SentenceTable:
    """dtk_sentence_view (datok_gpu.h): a batch's sentences as rows, under the C names.  A sentence is a maximal
    non-empty run of Token calls with no SentenceEnd / TextEnd between them; row i of document d holds the document's
    tokens [sen_tok_end[i - 1], sen_tok_end[i]) (0 at the document's first row), the bytes [sen_bstart[i], sen_bend[i])
    of the document and the runes [sen_rstart[i], sen_rend[i]) of the text.  Host table: numpy arrays (sen_rstart /
    sen_rend are None after a run with NO_RUNE_OFFSETS); device table: the raw device pointers as ints (or None)."""
    __slots__ = ("n_sen", "sen_off", "sen_tok_end", "sen_bstart", "sen_bend", "sen_rstart", "sen_rend", "text_sen_end")

    def doc(self, d):
        """The rows of document d of a host table."""
        a, b = int(self.sen_off[d]), int(self.sen_off[d + 1])
        return dict(sen_tok_end=self.sen_tok_end[a:b], sen_bstart=self.sen_bstart[a:b], sen_bend=self.sen_bend[a:b],
                    sen_rstart=None if self.sen_rstart is None else self.sen_rstart[a:b],
                    sen_rend=None if self.sen_rend is None else self.sen_rend[a:b])


def _pack_words(words):
    """A list of bytes objects as dtk_vocab_create takes it: the bytes back to back and n + 1 uint64 offsets."""
    words = [bytes(w) for w in words]
    off = np.zeros(len(words) + 1, np.uint64)
    if words:
        off[1:] = np.cumsum([len(w) for w in words], dtype=np.uint64)
    blob = np.frombuffer(b"".join(words), dtype=np.uint8) if int(off[-1]) else np.zeros(1, np.uint8)
    return blob, off, len(words)


class Vocab:
    """dtk_vocab: an ordered list of byte strings on the device; a token's id is the index of the word equal to its
    surface as the writer prints it (invalid bytes as U+FFFD), the lowest one of equal words, or -1.  Immutable and
    shareable between batches."""

    def __init__(self, words):
        blob, off, n = _pack_words(words)
        self._h = C.c_void_p()
        check(lib().dtk_vocab_create(blob.ctypes.data, off.ctypes.data, n, C.byref(self._h)), "dtk_vocab_create")

    @property
    def size(self):
        return int(lib().dtk_vocab_size(self._h))

    @staticmethod
    def probe(words, key: bytes) -> int:
        """dtk_vocab_probe_mem: the id of `key` (its bytes after replacement) in `words`, looked up on the host with the
        table and the probe the kernel uses.  Needs no device."""
        blob, off, n = _pack_words(words)
        key = bytes(key)
        kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
        out = C.c_int32(0)
        check(lib().dtk_vocab_probe_mem(blob.ctypes.data, off.ctypes.data, n, kb.ctypes.data, len(key), C.byref(out)),
              "dtk_vocab_probe_mem")
        return int(out.value)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_vocab_free(h)

    __del__ = close


class Tally:
    """dtk_tally: size + 1 exact 64-bit counters beside a vocabulary; every run of a batch, pipeline or stream it is
    attached to adds its tokens once, the unknown ones to the last counter."""

    def __init__(self, vocab: Vocab):
        self._h = C.c_void_p()
        self._vocab = vocab   # (kept alive)
        self.size = vocab.size
        check(lib().dtk_tally_create(vocab._h, C.byref(self._h)), "dtk_tally_create")

    def read(self) -> np.ndarray:
        out = np.zeros(self.size + 1, np.uint64)
        check(lib().dtk_tally_read(self._h, out.ctypes.data), "dtk_tally_read")
        return out

    def reset(self):
        check(lib().dtk_tally_reset(self._h), "dtk_tally_reset")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_tally_free(h)

    __del__ = close


def _set_vocab(fn, name, owner, v, tally, ids_home):
    check(fn(owner._h, v._h if v is not None else None, tally._h if tally is not None else None, 1 if ids_home else 0), name)
    owner._vocab = (v, tally)   # (they must outlive the owner's use of them)


def _set_wordpiece(fn, name, owner, v, prefix, unk_id, max_runes, pieces_home):
    prefix = bytes(prefix)
    pb = np.frombuffer(prefix, dtype=np.uint8) if prefix else np.zeros(1, np.uint8)
    check(fn(owner._h, v._h if v is not None else None, pb.ctypes.data, len(prefix), int(unk_id), int(max_runes),
             1 if pieces_home else 0), name)
    owner._wp_vocab = v   # (it must outlive the owner's use of it)


class Pieces:
    """A run's tokens split into WordPiece ids (dtk_piece_view): token i's pieces are piece_id[piece_off[i]:piece_off[i + 1]]
    (np.int32; piece_off np.uint64, n_tok + 1), piece_bend (np.uint32) each piece's end as a byte offset in its document,
    in source bytes; n_unknown counts the tokens that became the single unk_id piece."""
    __slots__ = ("piece_off", "piece_id", "piece_bend", "n_pieces", "n_unknown")

    def __init__(self, piece_off, piece_id, piece_bend, n_pieces, n_unknown):
        self.piece_off, self.piece_id, self.piece_bend = piece_off, piece_id, piece_bend
        self.n_pieces, self.n_unknown = n_pieces, n_unknown


def _pieces_of(v, copy=True) -> Pieces:
    """Host arrays of a dtk_piece_view whose pointers are host pointers."""
    def arr(ptr, n, dt):
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        a = np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt)
        return a.copy() if copy else a
    n_tok, n_pieces = int(v.n_tok), int(v.n_pieces)
    return Pieces(arr(v.piece_off, n_tok + 1, np.uint64), arr(v.piece_id, n_pieces, np.int32),
                  arr(v.piece_bend, n_pieces, np.uint32), n_pieces, int(v.n_unknown))


def _pack_fold(mapping):
    """A dict from code point to str (or to a sequence of code points) as dtk_fold_create takes it: (from, to_off, to, n)."""
    items = [(int(cp), [ord(c) for c in t] if isinstance(t, str) else [int(c) for c in t]) for cp, t in mapping.items()]
    frm = np.array([cp for cp, _ in items] or [0], np.uint32)
    to_off = np.zeros(len(items) + 1, np.uint32)
    if items:
        to_off[1:] = np.cumsum([len(t) for _, t in items], dtype=np.uint64)
    to = np.array([c for _, t in items for c in t] or [0], np.uint32)
    return frm, to_off, to, len(items)


class Fold:
    """dtk_fold: a finite map from a code point to 0..4 code points on the device, applied rune by rune to every token's
    key where the lookup (set_vocab) and the split (set_wordpiece) read it; offsets and piece ends stay in source bytes.
    `mapping`: a dict from code point to str; code points it does not list fold to themselves.  Immutable and shareable
    between batches.  The vocabulary is not folded: it must be in folded form already."""

    def __init__(self, mapping):
        frm, to_off, to, n = _pack_fold(mapping)
        self._h = C.c_void_p()
        check(lib().dtk_fold_create(frm.ctypes.data, to_off.ctypes.data, to.ctypes.data, n, C.byref(self._h)), "dtk_fold_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_fold_free(h)

    __del__ = close


def _set_fold(fn, name, owner, fold):
    check(fn(owner._h, fold._h if fold is not None else None), name)
    owner._fold = fold   # (it must outlive the owner's use of it)


def fold_apply(mapping, key: bytes) -> bytes:
    """dtk_fold_apply_mem: the folded key F(K) of `key` under `mapping` (a dict from code point to str), computed on the
    host with the tables the kernels use; bytes of `key` that do not decode fold as U+FFFD.  Needs no device."""
    frm, to_off, to, n = _pack_fold(mapping)
    key = bytes(key)
    kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
    out = np.zeros(max(16 * len(key), 1), np.uint8)
    n_out = C.c_size_t(0)
    check(lib().dtk_fold_apply_mem(frm.ctypes.data, to_off.ctypes.data, to.ctypes.data, n, kb.ctypes.data, len(key),
                                   out.ctypes.data, len(out), C.byref(n_out)), "dtk_fold_apply_mem")
    return out[:int(n_out.value)].tobytes()


_BERT_UNCASED = None


def bert_uncased_mapping():
    """The fold of BERT's uncased BasicTokenizer as a mapping for Fold, from the standard library's Unicode tables: for
    every scalar value c, F(c) is NFD(c.lower()) without the characters of category Mn; only c with F(c) != c are
    listed.  Per rune, like the `tokenizers` package: a final sigma, which str.lower() on a whole token treats by its
    context, folds like any other.  Built once and cached; the caller must not change it."""
    global _BERT_UNCASED
    if _BERT_UNCASED is None:
        import unicodedata
        m = {}
        for cp in range(0x110000):
            if 0xD800 <= cp <= 0xDFFF:
                continue
            c = chr(cp)
            f = "".join(x for x in unicodedata.normalize("NFD", c.lower()) if unicodedata.category(x) != "Mn")
            if f != c:
                m[cp] = f
        _BERT_UNCASED = m
    return _BERT_UNCASED


def wordpiece_probe(words, key: bytes, prefix=b"##", unk_id=0, max_runes=0, cap=None, fold=None):
    """dtk_wordpiece_probe_mem: `key` (its bytes after replacement) split over `words` on the host with the table and the
    rule the kernels use: (ids, ends), ends in key bytes.  Needs no device.  cap: room for that many pieces (default:
    enough); with more the call raises DatokGpuError E_CAPACITY whose .needed is the count.  fold: a mapping as Fold
    takes it (dtk_wordpiece_probe_fold_mem): the key, valid UTF-8, is read through it; ends stay in bytes of `key`."""
    if fold is not None:
        return _wordpiece_probe_fold(words, key, prefix, unk_id, max_runes, cap, fold)
    blob, off, n = _pack_words(words)
    key, prefix = bytes(key), bytes(prefix)
    kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
    pb = np.frombuffer(prefix, dtype=np.uint8) if prefix else np.zeros(1, np.uint8)
    room = len(key) + 1 if cap is None else int(cap)
    ids, ends = np.zeros(max(room, 1), np.int32), np.zeros(max(room, 1), np.uint32)
    n_out = C.c_uint32(0)
    rc = lib().dtk_wordpiece_probe_mem(blob.ctypes.data, off.ctypes.data, n, pb.ctypes.data, len(prefix), int(unk_id),
                                       int(max_runes), kb.ctypes.data, len(key), ids.ctypes.data, ends.ctypes.data, room,
                                       C.byref(n_out))
    if rc != _lib.OK:
        e = _lib.DatokGpuError(rc, "dtk_wordpiece_probe_mem")
        e.needed = int(n_out.value) if rc == _lib.E_CAPACITY else None
        raise e
    k = int(n_out.value)
    return ids[:k].copy(), ends[:k].copy()


def _wordpiece_probe_fold(words, key, prefix, unk_id, max_runes, cap, fold):
    blob, off, n = _pack_words(words)
    frm, to_off, to, n_fold = _pack_fold(fold)
    key, prefix = bytes(key), bytes(prefix)
    kb = np.frombuffer(key, dtype=np.uint8) if key else np.zeros(1, np.uint8)
    pb = np.frombuffer(prefix, dtype=np.uint8) if prefix else np.zeros(1, np.uint8)
    room = len(key) + 1 if cap is None else int(cap)
    ids, ends = np.zeros(max(room, 1), np.int32), np.zeros(max(room, 1), np.uint32)
    n_out = C.c_uint32(0)
    rc = lib().dtk_wordpiece_probe_fold_mem(blob.ctypes.data, off.ctypes.data, n, pb.ctypes.data, len(prefix), int(unk_id),
                                            int(max_runes), frm.ctypes.data, to_off.ctypes.data, to.ctypes.data, n_fold,
                                            kb.ctypes.data, len(key), ids.ctypes.data, ends.ctypes.data, room, C.byref(n_out))
    if rc != _lib.OK:
        e = _lib.DatokGpuError(rc, "dtk_wordpiece_probe_fold_mem")
        e.needed = int(n_out.value) if rc == _lib.E_CAPACITY else None
        raise e
    k = int(n_out.value)
    return ids[:k].copy(), ends[:k].copy()


def _encode_spec(max_len, cls_id, sep_id, pad_id, unit, stride, first_window, word_ids):
    units = {"sentence": _lib.ENC_SENTENCE, "document": _lib.ENC_DOCUMENT}
    flags = (_lib.ENC_FIRST_WINDOW if first_window else 0) | (_lib.ENC_WORD_IDS if word_ids else 0)
    return _lib.EncodeSpec(int(max_len), int(cls_id), int(sep_id), int(pad_id),
                           units[unit] if isinstance(unit, str) else int(unit), int(stride), flags)


def _set_encode(fn, name, owner, max_len, kw):
    spec = None if max_len is None else _encode_spec(max_len, kw["cls_id"], kw["sep_id"], kw["pad_id"], kw["unit"],
                                                     kw["stride"], kw["first_window"], kw["word_ids"])
    check(fn(owner._h, C.byref(spec) if spec is not None else None, 1 if kw["rows_home"] else 0), name)


class Encoded:
    """A run's sentences or documents as fixed-length model input rows (dtk_encode_view): row unit_row_off[u] + k is
    window k of unit u; input_ids (np.int32, (n_rows, max_len)): cls_id, the window's piece ids, sep_id, pad_id; row_len
    (np.uint32) the positions in front of the padding; row_piece0 (np.uint64) the batch-wide index into piece_id of the
    row's first body piece; word_id (np.int32, (n_rows, max_len), None without word_ids) the document-relative index of
    each body position's token, -1 elsewhere; n_cut counts the units with more pieces than a row's body holds."""
    __slots__ = ("unit_row_off", "input_ids", "row_len", "row_piece0", "word_id", "n_units", "n_rows", "n_cut", "max_len")

    def __init__(self, unit_row_off, input_ids, row_len, row_piece0, word_id, n_units, n_rows, n_cut, max_len):
        self.unit_row_off, self.input_ids, self.row_len, self.row_piece0, self.word_id = unit_row_off, input_ids, row_len, row_piece0, word_id
        self.n_units, self.n_rows, self.n_cut, self.max_len = n_units, n_rows, n_cut, max_len

    def attention_mask(self):
        """(n_rows, max_len) np.int32: 1 in front of the padding."""
        return (np.arange(self.max_len, dtype=np.uint32)[None, :] < self.row_len[:, None]).astype(np.int32)


def _encoded_of(v, copy=True) -> Encoded:
    """Host arrays of a dtk_encode_view whose pointers are host pointers."""
    def arr(ptr, n, dt):
        if n == 0 or not ptr:
            return np.zeros(0, dt)
        a = np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt)
        return a.copy() if copy else a
    nu, nr, ml = int(v.n_units), int(v.n_rows), int(v.max_len)
    return Encoded(arr(v.unit_row_off, nu + 1, np.uint64), arr(v.input_ids, nr * ml, np.int32).reshape(nr, ml),
                   arr(v.row_len, nr, np.uint32), arr(v.row_piece0, nr, np.uint64),
                   arr(v.word_id, nr * ml, np.int32).reshape(nr, ml) if v.word_id else None, nu, nr, int(v.n_cut), ml)


def encode_rows(piece_off, piece_id, unit_tok_end, max_len, cls_id, sep_id, pad_id, stride=0, first_window=False,
                word_ids=False, tok_off=None, cap_rows=None) -> Encoded:
    """dtk_encode_rows_mem: the encoding rule on the host, with the code the kernels run.  The units are token ranges:
    unit u is [unit_tok_end[u - 1], unit_tok_end[u]) batch-wide, from 0; tok_off is needed for word_ids.  Needs no
    device.  cap_rows: room for that many rows (default: enough); with more the call raises DatokGpuError E_CAPACITY
    whose .needed is the count."""
    piece_off = np.ascontiguousarray(piece_off, dtype=np.uint64)
    piece_id = np.ascontiguousarray(piece_id, dtype=np.int32)
    ends = np.ascontiguousarray(unit_tok_end, dtype=np.uint64)
    toff = None if tok_off is None else np.ascontiguousarray(tok_off, dtype=np.uint64)
    spec = _encode_spec(max_len, cls_id, sep_id, pad_id, _lib.ENC_DOCUMENT, stride, first_window, word_ids)
    n_tok, n_units = len(piece_off) - 1, len(ends)
    n_rows, n_cut = C.c_uint64(0), C.c_uint64(0)
    off = np.zeros(n_units + 1, np.uint64)
    ml = max(int(max_len), 1)

    def call(cap):
        ids = np.zeros((max(cap, 1), ml), np.int32)
        words = np.zeros((max(cap, 1), ml), np.int32) if word_ids else None
        rl, p0 = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64)
        rc = lib().dtk_encode_rows_mem(C.byref(spec), piece_off.ctypes.data, n_tok, piece_id.ctypes.data if len(piece_id) else None,
                                       ends.ctypes.data if n_units else None, n_units,
                                       toff.ctypes.data if toff is not None else None, 0 if toff is None else len(toff) - 1,
                                       cap, off.ctypes.data, ids.ctypes.data, rl.ctypes.data, p0.ctypes.data,
                                       words.ctypes.data if words is not None else None, C.byref(n_rows), C.byref(n_cut))
        return rc, ids, words, rl, p0
    rc, ids, words, rl, p0 = call(0 if cap_rows is None else int(cap_rows))
    if rc == _lib.E_CAPACITY and cap_rows is None:
        rc, ids, words, rl, p0 = call(int(n_rows.value))
    if rc != _lib.OK:
        e = _lib.DatokGpuError(rc, "dtk_encode_rows_mem")
        e.needed = int(n_rows.value) if rc == _lib.E_CAPACITY else None
        raise e
    n = int(n_rows.value)
    return Encoded(off, ids[:n], rl[:n], p0[:n], None if words is None else words[:n], n_units, n, int(n_cut.value), int(max_len))


class Batch:
    """dtk_batch: device buffers + one HIP stream for many documents per launch."""

    def __init__(self, max_bytes, max_docs):
        self._h = C.c_void_p()
        check(lib().dtk_batch_create(int(max_bytes), int(max_docs), C.byref(self._h)), "dtk_batch_create")
        self._keep = None
        self.n_docs = 0
        self.total = 0
        self._doc_off = None

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_batch_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self):
        return lib().dtk_batch_stream(self._h)

    def set_input(self, text: np.ndarray, doc_off: np.ndarray):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        self._keep = (text, doc_off)
        self.n_docs = len(doc_off) - 1
        self.total = int(doc_off[-1])
        self._doc_off = doc_off
        check(lib().dtk_batch_set_input(self._h, text.ctypes.data, doc_off.ctypes.data, self.n_docs),
              "dtk_batch_set_input")

    def set_input_device(self, d_text_ptr, d_doc_off_ptr, n_docs, total_bytes, keep=None, doc_off_host=None):
        """Device-resident input (e.g. torch tensors' data_ptr()); `keep` pins the owners."""
        check(lib().dtk_batch_set_input_device(self._h, d_text_ptr, d_doc_off_ptr, int(n_docs), int(total_bytes)),
              "dtk_batch_set_input_device")
        # (only now: a rejected call leaves the batch, and this object, with the input they had)
        self._keep = keep
        self.n_docs = int(n_docs)
        self.total = int(total_bytes)
        self._doc_off = doc_off_host

    def run(self, tok: Tokenizer, flags=0):
        check(lib().dtk_batch_run(tok._h, self._h, flags), "dtk_batch_run")

    def sync(self):
        check(lib().dtk_batch_sync(self._h), "dtk_batch_sync")

    AUTO_CHUNK = 0xFFFFFFFF

    def set_chunking(self, chunk_bytes=AUTO_CHUNK, warm_bytes=8, extend=None):
        """0: one lane per document; otherwise speculative chunk lanes (exact either way).
        extend: how far the warm-up start may move back to the previous blank (None: library default,
        0: fixed distance only -- what tests use to force mispredictions)."""
        check(lib().dtk_batch_set_chunking(self._h, int(chunk_bytes), int(warm_bytes)), "dtk_batch_set_chunking")
        if extend is not None:
            check(lib().dtk_batch_set_warm_extend(self._h, int(extend)), "dtk_batch_set_warm_extend")

    def set_profiling(self, enable=True):
        check(lib().dtk_batch_set_profiling(self._h, int(bool(enable))), "dtk_batch_set_profiling")

    STAGES = ("clear", "symbolize", "spec_start", "spec_link", "walk", "spec_verify", "spec_fix", "scan", "compact")

    def stage_ms(self):
        """Milliseconds per stage of the last run (needs set_profiling(True))."""
        ms = (C.c_float * 9)()
        check(lib().dtk_batch_stage_ms(self._h, C.byref(ms)), "dtk_batch_stage_ms")
        return dict(zip(self.STAGES, [float(x) for x in ms]))

    def totals(self):
        t = Totals()
        check(lib().dtk_batch_totals(self._h, C.byref(t)), "dtk_batch_totals")
        return {k: getattr(t, k) for k, _ in Totals._fields_}

    def debug_stream(self):
        """Test accessor (dtk_batch_debug_stream): what the symbolise kernel wrote in the last run, as (entries,
        rune_start_words, saw_invalid) -- uint16[total] entries `symbol | width << 11 | class << 14` in the model
        file's symbol numbering, the rune-start bitmap as uint32[(total + 31) // 32], and whether the run met an
        invalid UTF-8 byte."""
        entries = np.zeros(self.total, dtype=np.uint16)
        words = np.zeros((self.total + 31) // 32, dtype=np.uint32)
        saw = C.c_uint32(0)
        check(lib().dtk_batch_debug_stream(self._h, entries.ctypes.data, words.ctypes.data, C.byref(saw)),
              "dtk_batch_debug_stream")
        return entries, words, bool(saw.value)

    def result_device(self) -> ResultView:
        v = ResultView()
        check(lib().dtk_batch_result_device(self._h, C.byref(v)), "dtk_batch_result_device")
        return v

    def render_device(self, flags=SIMPLE) -> RenderView:
        """NewTokenWriter(w, flags) for every document, left on the device (pointers + total)."""
        v = RenderView()
        check(lib().dtk_batch_render_device(self._h, flags, C.byref(v)), "dtk_batch_render_device")
        return v

    def render(self, flags=SIMPLE):
        """Returns (bytes, doc_off): bytes[doc_off[d]:doc_off[d+1]] is what the reference writes for document d."""
        v = RenderView()
        check(lib().dtk_batch_render_host(self._h, flags, C.byref(v)), "dtk_batch_render_host")
        off = np.frombuffer((C.c_char * ((self.n_docs + 1) * 8)).from_address(v.doc_off), dtype=np.uint64).copy()
        data = C.string_at(v.bytes, v.total) if v.total else b""
        return data, off

    # dtk_batch_set_result_fields (datok_gpu.h DTK_R_*)
    R_CSR, R_TOK_RUNE, R_TOK_BYTE, R_SENT, R_TEXTS, R_STATUS, R_EVENTS, R_ALL = 1, 2, 4, 8, 16, 32, 64, 127
    R_TOK_RUNE16 = 128   # the rune offsets as int16 pairs (BatchResult.tok_r16); a batch with a document longer than
                         # 32 767 bytes gets tok_rstart / tok_rend in their place
    R_EAGER = 256        # the selected arrays leave for the host inside the run (k_to_host) where they fit
    R_TOK_RUNE_BLK = 512   # the rune / byte offsets as blocks of 64 tokens with 16-bit offsets (BatchResult.tok_rblk +
    R_TOK_BYTE_BLK = 1024  # tok_rblk_head / tok_bblk + tok_bblk_head, unpack_blocked): any document length; a batch with
                           # a block that does not fit gets the 32-bit arrays in their place
    R_EVENT_LIST = 2048    # what a closure replay needs of the event bitmaps as a list (BatchResult.evl_off / evl_pos /
                           # evl_kind, replay_list) + doc_tail: about one 5-byte entry per sentence

    R_SENTENCES = 8192     # the sentence table (sentences()) comes home with the download; without the bit it is built
                           # and copied when sentences() asks

    def sentences(self, device=False, copy=True) -> SentenceTable:
        """The last run's sentences as rows (dtk_batch_sentences_host; device=True: dtk_batch_sentences_device, the
        table stays in HBM and the fields are raw device pointers).  copy=False: views of the batch's page-locked
        block, valid until its next run.  E_STATE before a run and after a run with NO_BYTE_OFFSETS."""
        v = SentenceView()
        fn = lib().dtk_batch_sentences_device if device else lib().dtk_batch_sentences_host
        check(fn(self._h, C.byref(v)), "dtk_batch_sentences_device" if device else "dtk_batch_sentences_host")
        t = SentenceTable()
        t.n_sen = int(v.n_sen)
        names = [n for n, _ in SentenceView._fields_[1:]]
        if device:
            for n in names:
                setattr(t, n, getattr(v, n) or None)
            return t
        n_texts = self.totals()["n_texts"]
        shape = dict(sen_off=(self.n_docs + 1, np.uint64), sen_tok_end=(t.n_sen, np.uint32), sen_bstart=(t.n_sen, np.uint32),
                     sen_bend=(t.n_sen, np.uint32), sen_rstart=(t.n_sen, np.int32), sen_rend=(t.n_sen, np.int32),
                     text_sen_end=(n_texts, np.uint32))
        for n in names:
            ptr, (cnt, dt) = getattr(v, n), shape[n]
            if not ptr:
                setattr(t, n, None)
            elif cnt == 0:
                setattr(t, n, np.zeros(0, dt))
            else:
                a = np.frombuffer((C.c_char * (cnt * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt)
                setattr(t, n, a.copy() if copy else a)
        return t

    def set_vocab(self, v, tally=None, ids_home=True):
        """Every token of the next runs is looked up in the Vocab `v` (None: off) behind the run, on the download
        stream; `tally` (a Tally of v) gets each run's tokens once.  ids_home: the ids come home with the other result
        copies (download_begin / result); False: they stay in HBM until token_ids() asks."""
        _set_vocab(lib().dtk_batch_set_vocab, "dtk_batch_set_vocab", self, v, tally, ids_home)

    def token_ids(self, device=False, copy=True):
        """The last run's ids: (np.int32 array in the order tok_off indexes, n_unknown).  copy=False: a view of the batch's
        page-locked block, valid until its next run.  device=True: the raw dtk_token_id_view (tok_id is a device
        pointer).  E_STATE before a run, without a vocabulary and after a run with NO_BYTE_OFFSETS."""
        v = _lib.TokenIdView()
        fn = lib().dtk_batch_token_ids_device if device else lib().dtk_batch_token_ids_host
        check(fn(self._h, C.byref(v)), "dtk_batch_token_ids_device" if device else "dtk_batch_token_ids_host")
        if device:
            return v
        n = int(v.n_tok)
        if n == 0:
            return np.zeros(0, np.int32), int(v.n_unknown)
        a = np.frombuffer((C.c_char * (n * 4)).from_address(v.tok_id), dtype=np.int32)
        return (a.copy() if copy else a), int(v.n_unknown)

    def set_fold(self, fold):
        """dtk_batch_set_fold: the ids (set_vocab) and the split (set_wordpiece) read every key through `fold`
        (a Fold; None: off, the default).  A finished run's ids, pieces and rows are computed anew under it when they
        are next asked for."""
        _set_fold(lib().dtk_batch_set_fold, "dtk_batch_set_fold", self, fold)

    def set_wordpiece(self, v, prefix=b"##", unk_id=0, max_runes=0, pieces_home=True):
        """Every token of the next runs is split into WordPiece ids over the Vocab `v` (None: off) behind the run, on the
        download stream: greedy longest-match-first, continuation pieces looked up behind `prefix` (0..16 bytes), a token
        that cannot be split or has more than max_runes runes (0: 100) becomes the single piece unk_id.  pieces_home: the
        pieces come home with the other result copies; False: they stay in HBM until pieces() asks.  A vocabulary
        (set_vocab) may be attached beside it."""
        _set_wordpiece(lib().dtk_batch_set_wordpiece, "dtk_batch_set_wordpiece", self, v, prefix, unk_id, max_runes, pieces_home)

    def pieces(self, device=False, copy=True):
        """The last run's pieces: a Pieces.  copy=False: views of the batch's page-locked block, valid until its next
        run.  device=True: the raw dtk_piece_view (device pointers).  E_STATE before a run, without a split and after a
        run with NO_BYTE_OFFSETS."""
        v = _lib.PieceView()
        fn = lib().dtk_batch_pieces_device if device else lib().dtk_batch_pieces_host
        check(fn(self._h, C.byref(v)), "dtk_batch_pieces_device" if device else "dtk_batch_pieces_host")
        return v if device else _pieces_of(v, copy)

    def set_encode(self, max_len, cls_id=-1, sep_id=-1, pad_id=0, unit="sentence", stride=0, first_window=False,
                   word_ids=False, rows_home=True):
        """The next runs' sentences (unit="sentence") or documents ("document") become fixed-length model input rows
        behind the WordPiece split (set_wordpiece must be attached too): cls_id, the pieces, sep_id, pad_id up to
        max_len; -1 for cls_id / sep_id leaves the position out.  A unit with more pieces than a row's body is cut into
        windows that share `stride` pieces (first_window: only the first is kept).  word_ids: also each position's token.
        rows_home: the rows come home with the other result copies; False: they stay in HBM until encoded() asks.
        max_len=None turns it off."""
        _set_encode(lib().dtk_batch_set_encode, "dtk_batch_set_encode", self, max_len,
                    dict(cls_id=cls_id, sep_id=sep_id, pad_id=pad_id, unit=unit, stride=stride, first_window=first_window,
                         word_ids=word_ids, rows_home=rows_home))

    def encoded(self, device=False, copy=True):
        """The last run's model input rows: an Encoded.  copy=False: views of the batch's page-locked block, valid until
        its next run.  device=True: the raw dtk_encode_view (device pointers).  E_STATE before a run, without an
        encoding, without a split and after a run with NO_BYTE_OFFSETS."""
        v = _lib.EncodeView()
        fn = lib().dtk_batch_encoded_device if device else lib().dtk_batch_encoded_host
        check(fn(self._h, C.byref(v)), "dtk_batch_encoded_device" if device else "dtk_batch_encoded_host")
        return v if device else _encoded_of(v, copy)

    def set_result_fields(self, fields=R_ALL):
        """Which arrays result() brings to the host (the others come back empty)."""
        check(lib().dtk_batch_set_result_fields(self._h, int(fields)), "dtk_batch_set_result_fields")

    def download_begin(self):
        """Completes the run and starts the asynchronous copies of the selected arrays; result() waits for them."""
        check(lib().dtk_batch_download_begin(self._h), "dtk_batch_download_begin")

    def result(self, copy=True) -> BatchResult:
        """The result arrays on the host (dtk_batch_result_host).  copy=False: views of the batch's page-locked
        buffers, valid until its next run."""
        v = ResultView()
        check(lib().dtk_batch_result_host(self._h, C.byref(v)), "dtk_batch_result_host")
        t = self.totals()
        nd = self.n_docs

        def arr(ptr, n, dt):
            if n == 0 or not ptr:   # (an array that was not selected comes back NULL)
                return np.zeros(0, dt)
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr)
            a = np.frombuffer(buf, dtype=dt)
            return a.copy() if copy else a
        r = BatchResult()
        r.tok_off = arr(v.tok_off, nd + 1, np.uint64)
        r.sent_off = arr(v.sent_off, nd + 1, np.uint64)
        r.text_off = arr(v.text_off, nd + 1, np.uint64)
        r.tok_rstart = arr(v.tok_rstart, t["n_tokens"], np.int32)
        r.tok_rend = arr(v.tok_rend, t["n_tokens"], np.int32)
        r.tok_bstart = arr(v.tok_bstart, t["n_tokens"], np.uint32)
        r.tok_bend = arr(v.tok_bend, t["n_tokens"], np.uint32)
        r.sent = arr(v.sent, t["n_sent"], np.int32)
        r.text_tok_end = arr(v.text_tok_end, t["n_texts"], np.uint32)
        r.text_sent_end = arr(v.text_sent_end, t["n_texts"], np.uint32)
        r.status = arr(v.status, nd, np.uint32)
        r.ev_bits = arr(v.ev_bits, 5 * int(v.ev_words), np.uint32).reshape(5, -1) if v.ev_bits else np.zeros((5, 0), np.uint32)
        r.doc_tail = arr(v.doc_tail, nd, np.uint32)
        r.tok_r16 = arr(v.tok_r16, 2 * t["n_tokens"], np.int16).reshape(-1, 2)
        n_blk = (t["n_tokens"] + 63) // 64
        r.tok_rblk = arr(v.tok_rblk, t["n_tokens"], np.uint32)
        r.tok_rblk_head = arr(v.tok_rblk_head, 4 * n_blk, np.int32).reshape(-1, 4)
        r.tok_bblk = arr(v.tok_bblk, t["n_tokens"], np.uint32)
        r.tok_bblk_head = arr(v.tok_bblk_head, 4 * n_blk, np.int32).reshape(-1, 4)
        r.evl_off = arr(v.evl_off, nd + 1, np.uint32)
        n_evl = int(r.evl_off[-1]) if len(r.evl_off) else 0
        r.evl_pos = arr(v.evl_pos, n_evl, np.uint32)
        r.evl_kind = arr(v.evl_kind, n_evl, np.uint8)
        r.doc_off = self._doc_off
        r.exact = _exact_calls(v, arr)   # documents walked by the exact pass: id -> calls in order
        return r


class PinnedBuffer:
    """Page-locked host memory (dtk_pinned_alloc) as a numpy uint8 array: uploads from it are asynchronous."""

    def __init__(self, n):
        self._p = lib().dtk_pinned_alloc(int(n))
        if not self._p:
            raise MemoryError("dtk_pinned_alloc(%d)" % n)
        self.array = np.frombuffer((C.c_char * int(n)).from_address(self._p), dtype=np.uint8)

    def close(self):
        p, self._p = getattr(self, "_p", None), None
        if p:
            self.array = None
            lib().dtk_pinned_free(p)

    __del__ = close


class Pipeline:
    """dtk_pipeline: a corpus larger than one batch, cut into slices at document boundaries; the upload of one
    slice overlaps the walk of the others.  run() calls `on_slice(first_doc, n_docs, batch)` for every finished
    slice in order (batch: a Batch view of the slice, valid inside the callback)."""

    def __init__(self, slice_bytes, slice_docs, depth=3):
        self._h = C.c_void_p()
        check(lib().dtk_pipeline_create(int(slice_bytes), int(slice_docs), int(depth), C.byref(self._h)), "dtk_pipeline_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_pipeline_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_chunking(self, chunk_bytes=0xFFFFFFFF, warm_bytes=8):
        check(lib().dtk_pipeline_set_chunking(self._h, int(chunk_bytes), int(warm_bytes)), "dtk_pipeline_set_chunking")

    def set_vocab(self, v, tally=None, ids_home=True):
        """Batch.set_vocab for every slice: on_slice reads a slice's ids with batch.token_ids(); every slice's lookup
        has run when the slice is handed over, so a Tally holds the whole corpus when run() returns."""
        _set_vocab(lib().dtk_pipeline_set_vocab, "dtk_pipeline_set_vocab", self, v, tally, ids_home)

    def set_fold(self, fold):
        """Batch.set_fold for every slice."""
        _set_fold(lib().dtk_pipeline_set_fold, "dtk_pipeline_set_fold", self, fold)

    def set_wordpiece(self, v, prefix=b"##", unk_id=0, max_runes=0, pieces_home=True):
        """Batch.set_wordpiece for every slice: on_slice reads a slice's pieces with batch.pieces(); a slice is handed
        over when its split has finished."""
        _set_wordpiece(lib().dtk_pipeline_set_wordpiece, "dtk_pipeline_set_wordpiece", self, v, prefix, unk_id, max_runes,
                       pieces_home)

    def set_encode(self, max_len, cls_id=-1, sep_id=-1, pad_id=0, unit="sentence", stride=0, first_window=False,
                   word_ids=False, rows_home=True):
        """Batch.set_encode for every slice: on_slice reads a slice's rows with batch.encoded(); a slice is handed over
        when its encode has finished.  Units and row_piece0 count from 0 in every slice."""
        _set_encode(lib().dtk_pipeline_set_encode, "dtk_pipeline_set_encode", self, max_len,
                    dict(cls_id=cls_id, sep_id=sep_id, pad_id=pad_id, unit=unit, stride=stride, first_window=first_window,
                         word_ids=word_ids, rows_home=rows_home))

    def set_result_fields(self, fields):
        """Bring these result arrays (Batch.R_*) of every slice to the host, overlapped with the next slices' work."""
        check(lib().dtk_pipeline_set_result_fields(self._h, int(fields)), "dtk_pipeline_set_result_fields")

    def run(self, tok, text: np.ndarray, doc_off: np.ndarray, flags=0, on_slice=None):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        err = []
        fn = _slice_callback(on_slice, doc_off, err)
        rc = lib().dtk_pipeline_run(self._h, tok._h, text.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, flags, fn, None)
        if err:
            raise err[0]
        check(rc, "dtk_pipeline_run")


class Stream:
    """dtk_stream: ONE stream of any length, read through a reader and walked in slices of slice_bytes with bounded host
    memory (depth * (slice_bytes + 8192) page-locked bytes).  run() calls on_slice(SliceView) for every slice in order;
    the calls of the slices, one after the other, are the reference's calls for the whole stream (slice_calls,
    replay_slice)."""

    def __init__(self, slice_bytes=16 << 20, depth=3):
        self._h = C.c_void_p()
        check(lib().dtk_stream_create(int(slice_bytes), int(depth), C.byref(self._h)), "dtk_stream_create")
        self.slice_bytes = int(slice_bytes)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_stream_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_chunking(self, chunk_bytes=0xFFFFFFFF, warm_bytes=8):
        check(lib().dtk_stream_set_chunking(self._h, int(chunk_bytes), int(warm_bytes)), "dtk_stream_set_chunking")

    def set_result_fields(self, fields):
        """Batch.R_* of every slice's view: R_TOK_BYTE or R_TOK_BYTE_BLK, optionally R_EVENTS; the event list, the row
        offsets, the texts and the status always come."""
        check(lib().dtk_stream_set_result_fields(self._h, int(fields)), "dtk_stream_set_result_fields")

    def set_render(self, bits):
        """Every slice's SliceView.out: the bytes a stock NewTokenWriter(w, bits) writes for its calls, rendered on the
        device.  bits: TOKENS, SENTENCES, NEWLINE_AFTER_EOT (no effect); a position flag is E_ARG (those modes keep
        writer state across cuts: replay_slice).  None turns rendering off."""
        check(lib().dtk_stream_set_render(self._h, 0 if bits is None else 1, 0 if bits is None else int(bits)),
              "dtk_stream_set_render")

    def set_offsets(self, form):
        """Every SliceView brings the writer's rune offsets and sentence list as arrays (r_tok_rstart, r_tok_rend,
        r_sent, r_text_tok_end, r_text_sent_end, r_carry_in, r_carry_out): what a NewTokenWriter with TOKEN_POS |
        SENTENCE_POS -- and NEWLINE_AFTER_EOT iff run() gets it in its flags -- collects, carried from slice to slice on
        the device.  form: _lib.SO_PLAIN (int64 pairs) or _lib.SO_BLOCKED (16-bit blocks with 64-bit bases,
        unpack_blocked64); None turns it off.  Works beside set_render; E_ARG while set_position_render is on."""
        check(lib().dtk_stream_set_offsets(self._h, 0 if form is None else 1, 0 if form is None else int(form)),
              "dtk_stream_set_offsets")

    def set_vocab(self, v, tally=None, ids_home=True):
        """Every SliceView brings tok_id (np.int32, one per token of the slice: the slices' ids one behind the other are
        the ids of the stream as one document) and n_unknown; `tally` gets every slice's tokens once.  ids_home=False:
        tok_id stays None (a tally alone: nothing per token leaves the device).  None turns it off."""
        _set_vocab(lib().dtk_stream_set_vocab, "dtk_stream_set_vocab", self, v, tally, ids_home)

    def set_fold(self, fold):
        """Batch.set_fold for every slice of the stream."""
        _set_fold(lib().dtk_stream_set_fold, "dtk_stream_set_fold", self, fold)

    def set_wordpiece(self, v, prefix=b"##", unk_id=0, max_runes=0, pieces_home=True):
        """Every SliceView brings its tokens' pieces (piece_off from 0 in every slice, piece_id, piece_bend relative to the
        slice's window, n_pieces, n_piece_unknown): a token never spans a cut, so the slices' pieces one behind the other
        are the pieces of the stream as one document.  pieces_home=False: the arrays stay None, the counts come.  None
        turns it off."""
        _set_wordpiece(lib().dtk_stream_set_wordpiece, "dtk_stream_set_wordpiece", self, v, prefix, unk_id, max_runes,
                       pieces_home)

    def set_sentences(self, on):
        """Every SliceView brings the sentences its calls close as rows (s_tok_end, s_bstart, s_bend, s_rstart, s_rend,
        s_text_sen_end, s_carry_in, s_carry_out): the batch's sentence table for the stream as one document, the open
        row carried from slice to slice on the device.  Works alone (then the r_* fields stay None), beside set_offsets
        and beside set_render; E_ARG while set_position_render is on."""
        check(lib().dtk_stream_set_sentences(self._h, 1 if on else 0), "dtk_stream_set_sentences")

    def set_position_render(self, bits):
        """The same in a mode with TOKEN_POS or SENTENCE_POS (any of the five writer bits with one of the two): the
        writer's state is carried from slice to slice on the device, and every SliceView brings out, splice_pos,
        splice_sent, open_pos, open_sent, carry_in, carry_out and written.  run() must get the same NEWLINE_AFTER_EOT
        in its flags.  Turns set_render off (and set_render turns this off); None turns it off."""
        check(lib().dtk_stream_set_position_render(self._h, 0 if bits is None else 1, 0 if bits is None else int(bits)),
              "dtk_stream_set_position_render")

    @staticmethod
    def _reader_fn(reader, err):
        if not hasattr(reader, "read"):
            reader = io.BytesIO(reader.encode("utf-8") if isinstance(reader, str) else bytes(reader))

        def rd(_user, buf, cap):
            try:
                data = reader.read(cap)
                if isinstance(data, str):
                    raise TypeError("the reader must deliver bytes")
                if not data:
                    return 0
                C.memmove(buf, bytes(data), len(data))
                return len(data)
            except Exception as e:  # noqa: BLE001  (do not unwind through the C frame: the stream ends here)
                err.append(e)
                return 0
        return _lib.READ_FN(rd)

    def transduce(self, tok, reader, flags=SIMPLE):
        """dtk_stream_transduce: what the reference writes for the stream with a stock NewTokenWriter(w, flags) -- the
        slices' bytes as the device rendered them (with a position flag through dtk_stream_emit; both kinds of
        rendering are off afterwards).  Returns (output, status)."""
        err = []
        out, n, st = C.c_void_p(), C.c_size_t(), C.c_uint32()
        rc = lib().dtk_stream_transduce(self._h, tok._h, self._reader_fn(reader, err), None, int(flags), C.byref(out),
                                        C.byref(n), C.byref(st))
        if err:
            raise err[0]
        check(rc, "dtk_stream_transduce")
        try:
            return C.string_at(out, n.value), st.value
        finally:
            lib().dtk_free(out)

    def run(self, tok, reader, flags=0, on_slice=None) -> int:
        """reader: bytes, or an object with read(n) (b"" at the end; short reads are fine).  Returns the stream's status."""
        err = []
        rd = self._reader_fn(reader, err)

        def cb(_user, p):
            if on_slice is None:
                return 0
            try:
                on_slice(_slice_view(p.contents, self._h))
                return 0
            except Exception as e:  # noqa: BLE001
                err.append(e)
                return _lib.E_STATE
        st = C.c_uint32(0)
        rc = lib().dtk_stream_run(self._h, tok._h, rd, None, int(flags), _lib.STREAM_SLICE_FN(cb), None, C.byref(st))
        if err:
            raise err[0]
        check(rc, "dtk_stream_run")
        return int(st.value)


def _host_array(ptr, n, dt):
    """A copy of the n elements of dtype dt at the address ptr (none, or a null pointer: empty)."""
    dt = np.dtype(dt)
    if n == 0 or not ptr:
        return np.zeros(0, dt)
    return np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(ptr), dtype=dt).copy()


def _writer_carry(c):
    """A dtk_stream_pos_carry as a tuple: the writer's state at a cut."""
    return (int(c.posC), bool(c.sentB), bool(c.init), bool(c.pos_nonempty), bool(c.sent_nonempty))


def _slice_positions(h) -> dict:
    """What dtk_stream_positions and dtk_stream_emit say about the slice being delivered ({}: no position rendering)."""
    sp = _lib.StreamPos()
    if not h or lib().dtk_stream_positions(h, C.byref(sp)) != _lib.OK:
        return {}
    none = 2 ** 64 - 1
    parts = []

    def wr(_user, p, n):
        parts.append(C.string_at(p, n))
        return 0
    check(lib().dtk_stream_emit(h, _lib.WRITE_FN(wr), None), "dtk_stream_emit")
    return dict(splice_pos=None if sp.splice_pos == none else int(sp.splice_pos),
                splice_sent=None if sp.splice_sent == none else int(sp.splice_sent),
                open_pos=C.string_at(sp.open_pos, int(sp.open_pos_len)), open_sent=C.string_at(sp.open_sent, int(sp.open_sent_len)),
                carry_in=_writer_carry(sp.carry_in), carry_out=_writer_carry(sp.carry_out), written=b"".join(parts))


def _slice_offsets(h) -> dict:
    """What dtk_stream_offsets says about the slice being delivered ({}: offset delivery is off)."""
    so = _lib.StreamOffs()
    if not h or lib().dtk_stream_offsets(h, C.byref(so)) != _lib.OK:
        return {}
    arr = _host_array
    nt, ns, nx = int(so.n_tok), int(so.n_sent), int(so.n_text)
    blocked = not so.tok_rstart and bool(so.tok_rblk)
    words = heads = None
    if blocked:
        words, heads = arr(so.tok_rblk, nt, np.uint32), arr(so.tok_rblk_head, (nt + 63) // 64, HEAD64)
        rs, re = unpack_blocked64(words, heads)
    else:
        rs, re = arr(so.tok_rstart, nt, np.int64), arr(so.tok_rend, nt, np.int64)
    return dict(r_tok_rstart=rs, r_tok_rend=re, r_blocked=blocked, r_rblk=words, r_rblk_head=heads,
                r_sent=arr(so.sent, ns, np.int64), r_text_tok_end=arr(so.text_tok_end, nx, np.uint32),
                r_text_sent_end=arr(so.text_sent_end, nx, np.uint32), r_carry_in=_writer_carry(so.carry_in),
                r_carry_out=_writer_carry(so.carry_out))


def _slice_sentences(h) -> dict:
    """What dtk_stream_sentences says about the slice being delivered ({}: the sentence rows are off)."""
    ss = _lib.StreamSens()
    if not h or lib().dtk_stream_sentences(h, C.byref(ss)) != _lib.OK:
        return {}

    def carry(c):
        return (bool(c.open), int(c.bstart), int(c.bend), int(c.rstart), int(c.rend))
    arr = _host_array
    n, nx = int(ss.n_sen), int(ss.n_text)
    return dict(s_tok_end=arr(ss.sen_tok_end, n, np.uint32), s_bstart=arr(ss.sen_bstart, n, np.uint64),
                s_bend=arr(ss.sen_bend, n, np.uint64), s_rstart=arr(ss.sen_rstart, n, np.int64),
                s_rend=arr(ss.sen_rend, n, np.int64), s_text_sen_end=arr(ss.text_sen_end, nx, np.uint32),
                s_carry_in=carry(ss.carry_in), s_carry_out=carry(ss.carry_out))


def _slice_token_ids(h) -> dict:
    """What dtk_stream_token_ids says about the slice being delivered ({}: no vocabulary is attached)."""
    v = _lib.TokenIdView()
    if not h or lib().dtk_stream_token_ids(h, C.byref(v)) != _lib.OK:
        return {}
    return dict(tok_id=_host_array(v.tok_id, int(v.n_tok), np.int32) if v.tok_id or not v.n_tok else None,
                n_unknown=int(v.n_unknown))


def _slice_pieces(h) -> dict:
    """What dtk_stream_pieces says about the slice being delivered ({}: no split is attached)."""
    v = _lib.PieceView()
    if not h or lib().dtk_stream_pieces(h, C.byref(v)) != _lib.OK:
        return {}
    p = _pieces_of(v) if v.piece_off else None
    return dict(piece_off=p and p.piece_off, piece_id=p and p.piece_id, piece_bend=p and p.piece_bend,
                n_pieces=int(v.n_pieces), n_piece_unknown=int(v.n_unknown))


def _slice_view(s, stream=None) -> SliceView:
    """Host copies of a dtk_stream_slice (its buffers are only valid inside the callback)."""
    v = s.view
    arr = _host_array
    nt = int(arr(v.tok_off, 2, np.uint64)[1])
    if v.tok_bend:
        bs, be = arr(v.tok_bstart, nt, np.uint32), arr(v.tok_bend, nt, np.uint32)
    else:                                              # (R_TOK_BYTE_BLK)
        bs, be = (x.astype(np.uint32) for x in
                  unpack_blocked(arr(v.tok_bblk, nt, np.uint32), arr(v.tok_bblk_head, 4 * ((nt + 63) // 64), np.int32)))
    off = arr(v.evl_off, 2, np.uint32)
    ne = int(off[1])
    return SliceView(base=int(s.base), first=int(s.first), cut=int(s.cut), last=int(s.last), status=int(s.status),
                     text=C.string_at(s.text, int(s.len)) if s.len else b"",
                     tok_bstart=bs, tok_bend=be, evl_pos=arr(v.evl_pos, ne, np.uint32)[int(off[0]):],
                     evl_kind=arr(v.evl_kind, ne, np.uint8)[int(off[0]):], tail=int(arr(v.doc_tail, 1, np.uint32)[0]),
                     out=C.string_at(s.out, int(s.out_len)) if s.out else None, **_slice_positions(stream),
                     **_slice_offsets(stream), **_slice_sentences(stream), **_slice_token_ids(stream),
                     **_slice_pieces(stream))


def _slice_callback(on_slice, doc_off, err):
    """The C callback of dtk_pipeline_run / dtk_multi_run around a Python on_slice(first, n, batch_view)."""
    def cb(_user, first, n, handle):
        if on_slice is None:
            return 0
        view = Batch.__new__(Batch)
        try:
            view._h = C.c_void_p(handle); view._keep = None; view.n_docs = int(n)
            view._doc_off = (doc_off[first:first + n + 1] - doc_off[first]).astype(np.uint64)
            view.total = int(view._doc_off[-1])
            on_slice(int(first), int(n), view)
            return 0
        except Exception as e:  # noqa: BLE001  (do not unwind through the C frame)
            err.append(e)
            return _lib.E_STATE
        finally:
            # the pipeline owns the batch: the view must never free it, also not when on_slice raised and the
            # exception's traceback keeps the view alive (a double dtk_batch_free otherwise)
            view._h = None
    return _lib.SLICE_FN(cb)


class MultiPipeline:
    """dtk_multi: a corpus sharded over several GPUs of one node behind the C-ABI -- one worker thread, model replica
    and pipeline per listed device, slices dealt round-robin, finished slices handed to on_slice in corpus order."""

    def __init__(self, model_path, devices, slice_bytes, slice_docs, depth=3):
        self._h = C.c_void_p()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().dtk_multi_create(str(model_path).encode(), devs, len(devices), int(slice_bytes), int(slice_docs),
                                     int(depth), C.byref(self._h)), "dtk_multi_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib().dtk_multi_free(h)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def type(self):
        return lib().dtk_multi_type(self._h).decode()

    def set_result_fields(self, fields):
        check(lib().dtk_multi_set_result_fields(self._h, int(fields)), "dtk_multi_set_result_fields")

    def set_chunking(self, chunk_bytes=0xFFFFFFFF, warm_bytes=8):
        check(lib().dtk_multi_set_chunking(self._h, int(chunk_bytes), int(warm_bytes)), "dtk_multi_set_chunking")

    def run(self, text: np.ndarray, doc_off: np.ndarray, flags=0, on_slice=None):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        err = []
        fn = _slice_callback(on_slice, doc_off, err)
        rc = lib().dtk_multi_run(self._h, text.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, flags, fn, None)
        if err:
            raise err[0]
        check(rc, "dtk_multi_run")


def foma_to_matok(foma_gz: bytes) -> bytes:
    """`datok convert` (cmd/datok.go:50-70, matrix variant): LoadFomaFile + ToMatrix + Save.

    Takes the bytes of a gzip'd Foma text net and returns the bytes of the .matok file. Host only.
    """
    out, n = C.c_void_p(), C.c_size_t()
    check(lib().dtk_foma_to_matok(foma_gz, len(foma_gz), C.byref(out), C.byref(n)), "foma_to_matok")
    try:
        return C.string_at(out, n.value)
    finally:
        lib().dtk_free(out)


def foma_to_datok(foma_gz: bytes) -> bytes:
    """`datok convert --double-array` (cmd/datok.go:50-70): LoadFomaFile + ToDoubleArray (datok.go:82-238) + Save.

    The reference's layout depends on Go's map iteration order; this one takes a state's symbols in ascending order.
    Host only.
    """
    out, n = C.c_void_p(), C.c_size_t()
    check(lib().dtk_foma_to_datok(foma_gz, len(foma_gz), C.byref(out), C.byref(n)), "foma_to_datok")
    try:
        return C.string_at(out, n.value)
    finally:
        lib().dtk_free(out)


def model_info(gz_bytes: bytes) -> dict:
    """dtk_model_info_mem: what Tokenizer.info would say for this image (.matok, .datok or Foma net) -- kind, states,
    the device table's cell size (`entry_bytes`: 4 fused cells with 15-bit state ids, 8 fused 64-bit cells from 32 767
    states on), `dense_states`, `stream_codes` (0: the stream holds 16-bit entries), `lean_walk` (1: the lean loop walks
    it), `device_bytes` -- decided exactly as the loader decides it.  Host only:
    needs no device.  Raises DatokGpuError (E_FORMAT, E_MODEL) for an image the loader would reject."""
    info = ModelInfo()
    check(lib().dtk_model_info_mem(bytes(gz_bytes), len(gz_bytes), C.byref(info)), "model_info")
    return {k: getattr(info, k) for k, _ in ModelInfo._fields_}


def load_foma_file(path):
    """LoadFomaFile(path).ToMatrix() (fomafile.go:56-75, matrix.go:30-99) on the device."""
    return load_tokenizer_file(path)
