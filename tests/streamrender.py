"""The reference of the stream renderer (test infrastructure): tests/test_stream_render_host.py, tests/test_stream_render.py.

render_slice_ref states in numpy what dtk_streamrender.hip computes for one slice of a stream in a position-free writer
mode: the merge of the slice's tokens with its event list, and the size of every piece.
"""
import numpy as np

from datok_amd.host import (EVL_SEOT, EVL_SEPS, EVL_TEOT, SENTENCES, TOKEN_POS, SENTENCE_POS, TOKENS, _decode_runes,
                            _runes_to_bytes)

FFFD = b"\xef\xbf\xbd"


def invalid_flags(surface):
    """Per byte of `surface`: it does not decode (Go's rune iteration gives it U+FFFD of width 1)."""
    flags, i = [], 0
    for r in _decode_runes(surface):
        bad = r == 0xFFFD and surface[i:i + 3] != FFFD
        w = 1 if bad else len(chr(r).encode("utf-8"))
        flags += [bad] + [False] * (w - 1)
        i += w
    assert i == len(surface)
    return flags


def expand_ref(out, o, surface, invalid, cap):
    """The byte rule both renderers share (sym_expand, dtk_device.h): writes `surface` into the bytearray `out` from
    offset o on, a byte whose flag in `invalid` is set as U+FFFD, and stores nothing at or behind `cap` -- a replacement
    only if its three bytes fit, a plain byte only if it fits.  Returns the offset behind the surface, which does not
    depend on cap."""
    for b, bad in zip(surface, invalid):
        if bad:
            if o + 3 <= cap:
                out[o:o + 3] = FFFD
            o += 3
        else:
            if o < cap:
                out[o] = b
            o += 1
    return o


def _exclusive(w):
    out = np.zeros(len(w) + 1, dtype=np.int64)
    np.cumsum(w, out=out[1:])
    return out


def render_slice_ref(is_matrix, sl, bits) -> bytes:
    """What NewTokenWriter(w, bits) writes for the calls of the slice `sl` (a SliceView), bits without a position flag.

    Tokens and list entries are merged by cursor; at one cursor SEOT, TEOT, the token that ends there, SEPS; on the
    last slice the tail word's SentenceEnd and TextEnd follow everything else.  Sizes: a token under TOKENS is its
    surface (an input byte that does not decode prints as U+FFFD: two bytes more) and a newline; a SentenceEnd call is
    a newline under SENTENCES; a TextEnd call is a newline.  (is_matrix changes the calls' int arguments only, which no
    position-free mode reads.)"""
    assert not bits & (TOKEN_POS | SENTENCE_POS)
    tok, sen = 1 if bits & TOKENS else 0, 1 if bits & SENTENCES else 0
    text = sl.text
    bs, be = np.asarray(sl.tok_bstart, dtype=np.int64), np.asarray(sl.tok_bend, dtype=np.int64)
    pos, kind = np.asarray(sl.evl_pos, dtype=np.int64), np.asarray(sl.evl_kind, dtype=np.int64)
    surf = [_runes_to_bytes(_decode_runes(text[int(a):int(z)])) for a, z in zip(bs, be)] if tok else [b""] * len(bs)
    if tok:
        invalid = np.array([s.count(FFFD) - text[int(a):int(z)].count(FFFD) for s, a, z in zip(surf, bs, be)], dtype=np.int64)
        w_tok = be - bs + 2 * invalid + 1
        assert [len(s) + 1 for s in surf] == w_tok.tolist()
    else:
        w_tok = np.zeros(len(bs), dtype=np.int64)
    pre = ((kind & EVL_SEOT) != 0) * sen + ((kind & EVL_TEOT) != 0) * 1      # in front of a token on the same cursor
    post = ((kind & EVL_SEPS) != 0) * sen                                      # behind it
    tw, ew = _exclusive(w_tok), _exclusive(pre + post)
    lb = np.searchsorted(pos, be, side="left")                                 # the first entry at or behind the token's end
    same = (lb < len(pos)) & (pos[np.minimum(lb, max(len(pos) - 1, 0))] == be) if len(pos) else np.zeros(len(be), bool)
    off = tw[:-1] + ew[lb] + np.where(same, pre[np.minimum(lb, max(len(pos) - 1, 0))] if len(pos) else 0, 0)
    total = int(tw[-1] + ew[-1])
    if sl.last:
        tail = int(sl.tail)
        total += (sen if tail & 1 else 0) + (1 if tail & 2 else 0)
    out = bytearray(b"\n" * total)
    if tok:
        for o, a, z, s in zip(off.tolist(), bs.tolist(), be.tolist(), surf):
            piece = text[a:z]
            if piece.isascii():        # (every byte decodes and fits: the rule's plain case, without the loop)
                out[o:o + len(s)] = s
                continue
            assert expand_ref(out, o, piece, invalid_flags(piece), total) == o + len(s) and out[o:o + len(s)] == s
    assert len(out) == total
    return bytes(out)
