"""The reference of the stream renderer's position modes (test infrastructure): tests/test_stream_positions_host.py,
tests/test_stream_positions.py.

render_slice_pos_ref states in plain Python what dtk_streampos.hip computes for one slice of a stream in a writer mode
with TOKEN_POS or SENTENCE_POS: the slice's calls (tokens merged with the event list by cursor), the writer's rules
(token_writer.go:36-175, with the C++ mirror's answer to an empty text: the push is skipped and an empty list prints no
line), and the state that crosses the cut.  emit_ref is dtk_stream_emit: the splice of the held prefixes.
"""
from datok_amd.host import (EVL_SEOT, EVL_SEPS, EVL_TEOT, NEWLINE_AFTER_EOT, SENTENCES, SENTENCE_POS, TOKEN_POS, TOKENS,
                            TokenWriter, _decode_runes, _runes_to_bytes)

NONE = None                              # no splice offset (UINT64_MAX in the C-ABI)
CARRY0 = (0, True, True, False, False)   # posC, sentB, init, pos non-empty, sent non-empty: a fresh writer


def render_slice_pos_ref(is_matrix, sl, bits, carry_in):
    """(out, splice_pos, splice_sent, open_pos, open_sent, carry_out) of the slice `sl` (a SliceView) for a writer that
    enters it in the state carry_in = (posC, sentB, init, pos non-empty, sent non-empty).

    out: the bytes written during the slice's calls, where a position line holds the integers pushed in this slice only
    (each behind a blank if the line already has one) and the integers of the text still open at the cut are left out:
    they are open_pos / open_sent.  splice_pos / splice_sent: where in `out` the line of a text that began in an earlier
    slice starts (NONE: there is none)."""
    assert bits & (TOKEN_POS | SENTENCE_POS)
    posC, sentB, init, pne, sne = carry_in
    nl = bool(bits & NEWLINE_AFTER_EOT)
    text, n = sl.text, len(sl.text)
    out = bytearray()
    pos_line, sent_line = [], []               # this slice's integers of the current text
    cont_pos, cont_sent = pne, sne             # ... whose line has integers of earlier slices
    splice_pos = splice_sent = NONE

    def runes(a, z):
        return len(_decode_runes(text[a:z]))

    def line(ints, cont):
        return ((" " if cont and ints else "") + " ".join(map(str, ints))).encode()

    def sentence_end():
        nonlocal sentB, sne
        if bits & SENTENCE_POS:
            if pne:
                sent_line.append(posC)         # pos.back() == posC
                sne = True
            sentB = True
        if bits & SENTENCES:
            out.append(10)

    def text_end():
        nonlocal posC, pne, sne, sentB, cont_pos, cont_sent, splice_pos, splice_sent
        if bits & TOKEN_POS and pne:
            if cont_pos:
                splice_pos = len(out)
            out.extend(line(pos_line, cont_pos) + b"\n")
        if bits & SENTENCE_POS:
            if sne:
                if cont_sent:
                    splice_sent = len(out)
                out.extend(line(sent_line, cont_sent) + b"\n")
            sent_line.clear()
            sne, sentB, cont_sent = False, True, False
        posC, pne, cont_pos = 0, False, False
        pos_line.clear()

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
            sentence_end()
        if e & EVL_TEOT:
            text_end()
            if is_matrix:
                B = p
        if pt == p:
            start = int(sl.tok_bstart[k])
            k += 1
            if posC == 0 and nl and text[B] == 10 and not init:
                posC -= 1
            init = False
            posC += runes(B, start)
            pos_line.append(posC)
            pne = True
            if sentB:
                sentB = False
                sent_line.append(posC)
                sne = True
            posC += runes(start, p)
            pos_line.append(posC)
            if bits & TOKENS:
                out.extend(_runes_to_bytes(_decode_runes(text[start:p])) + b"\n")
            B = p
        if e & EVL_SEPS:
            sentence_end()
    if sl.last:
        if int(sl.tail) & 1:
            sentence_end()
        if int(sl.tail) & 2:
            text_end()
    open_pos = line(pos_line, cont_pos) if bits & TOKEN_POS else b""
    open_sent = line(sent_line, cont_sent) if bits & SENTENCE_POS else b""
    return bytes(out), splice_pos, splice_sent, open_pos, open_sent, (posC, sentB, init, pne, sne)


def emit_ref(held, r) -> bytes:
    """dtk_stream_emit: the slice's final bytes from render_slice_pos_ref's result `r` and the held prefixes
    held = [bytearray, bytearray] (TOKEN_POS, SENTENCE_POS), which take the slice's open fragments afterwards."""
    out, sp, ss, open_pos, open_sent, _ = r
    w = bytearray()
    at = 0
    for splice, h in ((sp, held[0]), (ss, held[1])):
        if splice != NONE:
            assert at <= splice <= len(out)
            w += out[at:splice] + h
            at = splice
            h.clear()
    w += out[at:]
    held[0] += open_pos
    held[1] += open_sent
    return bytes(w)


def mirror_token_writer(w, flags):
    """NewTokenWriter of the C++ mirror (include/datok.hpp:244-319) in a position mode: where the reference panics on an
    empty text (token_writer.go:108,135,145) it skips the push and prints no line for an empty list.  Returns (writer,
    its state: for the tests to read posC)."""
    assert flags & (TOKEN_POS | SENTENCE_POS)
    st = {"posC": 0, "pos": [], "sentB": True, "sent": [], "init": True}
    tw = TokenWriter()

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
            w.write(_runes_to_bytes(buf[offset:]) + b"\n")

    def sentence_end(_):
        if flags & SENTENCE_POS:
            if st["pos"]:
                st["sent"].append(st["pos"][-1])
            st["sentB"] = True
        if flags & SENTENCES:
            w.write(b"\n")

    def text_end(_):
        if flags & TOKEN_POS and st["pos"]:
            w.write(" ".join(map(str, st["pos"])).encode() + b"\n")
        if flags & SENTENCE_POS:
            if st["sent"]:
                w.write(" ".join(map(str, st["sent"])).encode() + b"\n")
            st["sent"] = []
            st["sentB"] = True
        st["posC"] = 0
        st["pos"] = []
    tw.Token, tw.SentenceEnd, tw.TextEnd, tw.Flush = token, sentence_end, text_end, lambda: None
    return tw, st
