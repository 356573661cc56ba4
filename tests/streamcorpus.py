"""Corpora and comparisons of the stream tests (test infrastructure): tests/test_stream_host.py, tests/test_stream.py.

A stream is ONE reader's bytes, texts separated by U+0004 (cmd/datok.go:120-133).  The reference for every comparison
is the oracle on the whole stream: its call list (oracle.Model.events) and its writer bytes (oracle.Model.transduce).
"""
import ctypes as C

import numpy as np

from datok_amd import corpus
from datok_amd.host import EVL_SEOT, EVL_SEPS, EVL_TEOT, SliceView, slice_calls

S, T = 16384, 8192          # the tests' slice size and the streamer's look-ahead tail (dtk_streamer.cpp)
MODES = list(range(16))     # TOKENS | SENTENCES | TOKEN_POS | SENTENCE_POS, with and without NEWLINE_AFTER_EOT (16)
ST_WINDOW_OVERFLOW, ST_EMPTY_TEXT = 1, 2


def running_text(total, seed=5, lang="de", text_bytes=9000):
    """`total` bytes of running text in several texts: generated documents joined by EOT + newline, cut on a blank."""
    n = total // text_bytes + 2
    if lang == "de":
        text, off = corpus.german_docs(n, text_bytes, seed=seed)
    else:
        text, off = corpus.english_zipf_docs(n, seed=seed, min_bytes=text_bytes, max_bytes=text_bytes)
    raw = bytes(text)
    docs = [raw[int(off[i]):int(off[i + 1])].rstrip() for i in range(len(off) - 1)]
    out = b"\x04\n".join(docs)
    assert len(out) >= total
    out = out[:total]
    cut = out.rfind(b" ")
    return out[:cut] + b"." * (total - cut)


# ---- a construct laid across byte S of a 40 KB stream
def _word4(n_runes):
    return ("\U00010330" * n_runes).encode()     # GOTHIC LETTER AHSA: four bytes a rune


#              name: (bytes, index of the byte of the construct that lies AT stream byte S when nothing is shifted)
CONSTRUCTS = {
    "rune3": ("Der Preis € hier.".encode(), 11),             # byte S is the middle byte of the 3-byte rune
    "eot_before": (b"Ende.\x04\nNeu hier ", 6),                    # EOT at S - 1
    "eot_at": (b"Ende.\x04\nNeu hier ", 5),                        # EOT at S
    "eot_after": (b"Ende.\x04\nNeu hier ", 4),                     # EOT at S + 1
    "sentence_end": (b"Das ist so. Und weiter ", 10),              # the full stop at S
    "token300": (b"a" * 300 + b" ", 150),                          # a blank-free token longer than any chunk
    "blanks600": (b" " * 600, 300),
    "token4000": (_word4(1000) + b" ", 8),                         # 4000 bytes in 1000 runes: the carried position sits near the tail's end
    "token5000": (b"a" * 5000 + b" ", 8),                          # more than a window holds: WINDOW_OVERFLOW, as the oracle reports
}
STREAM_40K = 40 * 1024
_filler = {}


def construct_stream(name, shift, total=STREAM_40K):
    """The construct in running text, its marked byte at stream byte S + shift (shift: leading blanks)."""
    body, at = CONSTRUCTS[name]
    if "f" not in _filler:
        _filler["f"] = running_text(total + 1024, seed=9)
    fill = _filler["f"]
    n_left = S - at
    left = fill[:n_left]
    cut = left.rfind(b" ")
    left = left[:cut] + b" " * (n_left - cut)
    out = b" " * shift + left + body
    right = fill[n_left:]
    right = right[right.find(b" "):]
    out += right[:total - len(out)]
    assert len(out) == total and out[shift + S - at:shift + S - at + len(body)] == body
    return out


# ---- the oracle's calls
class _Ev(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("a", C.c_int32), ("b", C.c_uint32), ("c", C.c_uint32), ("d", C.c_uint32)]


def oracle_calls(om, raw: bytes):
    """(calls, status): [(0, offset, window start, token start, token end) | (1, int) | (2, int)] in stream bytes; the
    status with what the position writer adds to the walk's (DTK_ST_EMPTY_TEXT: transduce_doc)."""
    ev, st = om.events(raw)
    return [(0, a, b, c, d) if k == 0 else (k, a) for k, a, b, c, d in ev], st | om.transduce_doc(raw).status


def stream_calls(is_matrix, slices):
    """The same list from the slices of a stream, one after the other."""
    from datok_amd.host import _decode_runes
    out = []
    for sl in slices:
        base, text = sl.base, sl.text
        for c in slice_calls(is_matrix, sl):
            if c[0] == "T":
                _, B, start, end = c
                out.append((0, len(_decode_runes(text[B:start])), base + B, base + start, base + end))
            else:
                kind, B, p, counted = c
                out.append((1 if kind == "S" else 2, len(_decode_runes(text[B:p])) if counted else 0))
    return out


def check_slices(slices, total, slice_bytes=S):
    """What holds for the slices of any stream: windows S apart, each beginning where its predecessor's cut lies."""
    assert slices and slices[-1].last and not any(s.last for s in slices[:-1])
    for k, s in enumerate(slices):
        assert s.base == k * slice_bytes
        assert s.first == (slices[k - 1].cut - slice_bytes if k else 0)
        if not s.last:
            assert len(s.text) == slice_bytes + T and slice_bytes <= s.cut < slice_bytes + 4104
        else:
            assert s.cut == len(s.text)
        assert s.first < 4104 and s.first <= s.cut
        if len(s.tok_bend):
            assert s.first < int(s.tok_bend[0]) and int(s.tok_bend[-1]) <= s.cut
            assert s.first <= int(s.tok_bstart[0])
        if len(s.evl_pos):
            assert s.first <= int(s.evl_pos[0]) and int(s.evl_pos[-1]) <= s.cut
    if slices[-1].status & ST_WINDOW_OVERFLOW == 0:
        assert slices[-1].base + len(slices[-1].text) == total


# ---- synthetic slices from the oracle's calls (CPU tier)
def _rune_starts(raw):
    a = np.frombuffer(raw, dtype=np.uint8)
    return np.flatnonzero((a & 0xC0) != 0x80)       # (well-formed UTF-8 only)


def calls_to_arrays(is_matrix, raw: bytes, calls):
    """(tok_bstart, tok_bend, [(cursor, EVL kind)], tail word) of one document from the oracle's calls: where the
    walk's bitmaps would hold them.  The cursor of a SentenceEnd / TextEnd comes from its int argument (runes since
    the window start) where the reference passes one, else from the call order."""
    starts = _rune_starts(raw)
    n = len(raw)

    def advance(B, a):
        i = int(np.searchsorted(starts, B)) + a
        return int(starts[i]) if i < len(starts) else n
    bs, be, ent = [], [], {}
    B = eot_from = 0
    tail = 0
    n_tok_left = sum(1 for c in calls if c[0] == 0)
    for i, c in enumerate(calls):
        if c[0] == 0:
            bs.append(c[3]); be.append(c[4]); B = c[4]; n_tok_left -= 1
            continue
        kind, a = c
        nxt_eot = raw.find(b"\x04", eot_from) + 1          # cursor behind the next EOT that has not fired (0: none)
        if kind == 2:
            p = nxt_eot if nxt_eot and (not is_matrix or advance(B, a) == nxt_eot) else 0
            if p:
                ent[p] = ent.get(p, 0) | EVL_TEOT
                eot_from = p
                if is_matrix:
                    B = p
            else:
                tail |= 2
        else:
            nxt = calls[i + 1] if i + 1 < len(calls) else None
            at_eot = nxt_eot and nxt is not None and nxt[0] == 2 and advance(B, a) == nxt_eot and (is_matrix or a > 0)
            if at_eot:
                ent[nxt_eot] = ent.get(nxt_eot, 0) | EVL_SEOT
            elif (n_tok_left == 0 and not nxt_eot and all(x[0] == 2 for x in calls[i + 1:])
                  and (not is_matrix or advance(B, a) == n)):
                tail |= 1        # the final SentenceEnd (an epsilon one at the very end replays the same)
            else:
                p = advance(B, a) if is_matrix else B
                assert not ent.get(p, 0) & EVL_SEPS
                ent[p] = ent.get(p, 0) | EVL_SEPS
    if tail:
        tail |= n << 2
    return np.array(bs, np.uint32), np.array(be, np.uint32), sorted(ent.items()), tail


def synthetic_slices(is_matrix, raw: bytes, calls, slice_bytes):
    """Cuts a document's calls into slice views as dtk_stream_run delivers them: window k begins at k * slice_bytes,
    and its cut is the first rewind (a token's end; for the matrix also a TextEnd fired by an EOT) at or behind its
    byte slice_bytes.  At the cut the closing kinds (token end, SEOT, TEOT) stay, the opening kind (SEPS) moves on."""
    bs, be, ent, tail = calls_to_arrays(is_matrix, raw, calls)
    rewinds = sorted(set(be.tolist()) | {p for p, k in ent if is_matrix and k & EVL_TEOT})
    out, first_abs, k = [], 0, 0
    while True:
        base = k * slice_bytes
        nxt = [p for p in rewinds if p >= base + slice_bytes]
        last = len(raw) <= base + slice_bytes + T or not nxt
        cut_abs = len(raw) if last else nxt[0]
        hi_close = len(raw) if last else cut_abs
        tsel = (be > first_abs) & (be <= hi_close) if k else (be <= hi_close)
        pos, kind = [], []
        for p, kd in ent:
            keep = 0
            if first_abs < p <= hi_close or (k == 0 and p <= hi_close):
                keep |= kd & (EVL_SEOT | EVL_TEOT)
            if (first_abs <= p < cut_abs) or (last and p == cut_abs and p >= first_abs):
                keep |= kd & EVL_SEPS
            if keep:
                pos.append(p - base); kind.append(keep)
        out.append(SliceView(base=base, first=first_abs - base, cut=cut_abs - base, last=int(last), status=0,
                             text=raw[base:base + slice_bytes + T],
                             tok_bstart=bs[tsel] - base, tok_bend=be[tsel] - base,
                             evl_pos=np.array(pos, np.uint32), evl_kind=np.array(kind, np.uint8),
                             tail=((tail >> 2) - base) << 2 | (tail & 3) if last and tail else 0))
        if last:
            return out
        first_abs = cut_abs
        k += 1
