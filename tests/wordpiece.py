"""The definition of a token's WordPiece split in plain Python (test infrastructure): tests/test_wordpiece_host.py,
tests/test_wordpiece.py.  It restates include/datok_gpu.h (dtk_batch_set_wordpiece); the keys are those of tests/tokenids.py.

A split takes a vocabulary (an ordered list of byte strings; of equal words the lowest index wins), a continuation
prefix, an unk_id and max_runes (0: 100).  For a key K, valid UTF-8:
  no key (None)                      one piece, unk_id
  K empty                            no piece
  more than max_runes runes          one piece, unk_id
  otherwise, start = 0, until start == len(K): the largest end > start on a rune boundary of K with
      K[start:end] (start == 0) or prefix + K[start:end] (otherwise) in the vocabulary gives a piece and start = end;
      without such an end the whole token is the single piece unk_id.
"""
import numpy as np

import tokenids

DEFAULT_RUNES = 100
REPL = b"\xef\xbf\xbd"


def rune_ends(key: bytes):
    """The offsets in (0, len(key)] at which a rune of `key` ends: where the next byte is no continuation byte."""
    return [e for e in range(1, len(key) + 1) if e == len(key) or (key[e] & 0xC0) != 0x80]


def split_key(words, key, prefix=b"##", unk_id=0, max_runes=0):
    """(pieces, unknown): pieces is a list of (id, end) with end an offset in KEY bytes; unknown says that the token
    became the single piece unk_id (its end is len(key), or 0 without a key)."""
    if key is None:
        return [(unk_id, 0)], True
    key = bytes(key)
    d = tokenids.vocab_dict(words)
    ends = rune_ends(key)
    if len(ends) > (max_runes or DEFAULT_RUNES):
        return [(unk_id, len(key))], True
    out, start = [], 0
    while start < len(key):
        for end in reversed([e for e in ends if e > start]):
            w = key[start:end] if start == 0 else bytes(prefix) + key[start:end]
            if w in d:
                out.append((d[w], end))
                start = end
                break
        else:
            return [(unk_id, len(key))], True
    return out, False


def source_offset(doc: bytes, bstart: int, bend: int, key_end: int):
    """Where key offset `key_end` of the row's key lies in the document, in source bytes: a byte that does not decode
    is one source byte and three key bytes (tokenids.key_of).  Piece ends lie on rune boundaries, so the walk meets
    key_end exactly."""
    seg = doc[bstart:bend]
    k = i = 0
    while k < key_end:
        for w in (1, 2, 3, 4):                                       # the rune at i, if one decodes there
            try:
                if len(seg[i:i + w].decode("utf-8")) == 1:
                    break
            except UnicodeDecodeError:
                pass
        else:
            w = 0
        i, k = (i + w, k + w) if w else (i + 1, k + 3)               # or one undecodable byte: EF BF BD
    assert k == key_end, (k, key_end)
    return bstart + i


def expected_pieces(words, text, doc_off, tok_off, tok_bstart, tok_bend, prefix=b"##", unk_id=0, max_runes=0):
    """(piece_off uint64, piece_id int32, piece_bend uint32, n_unknown) of a batch, from the arrays one run delivered."""
    raw = bytes(text)
    keys = tokenids.keys_of_batch(text, doc_off, tok_off, tok_bstart, tok_bend)
    off, ids, bends, n_unknown = [0], [], [], 0
    memo = {}
    for d in range(len(doc_off) - 1):
        doc = raw[int(doc_off[d]):int(doc_off[d + 1])]
        for i in range(int(tok_off[d]), int(tok_off[d + 1])):
            key = keys[i]
            if key not in memo:
                memo[key] = split_key(words, key, prefix, unk_id, max_runes)
            pieces, unknown = memo[key]
            bs, be = int(tok_bstart[i]), min(int(tok_bend[i]), len(doc))
            bs = min(bs, be) if key is not None else bs
            n_unknown += unknown
            for pid, end in pieces:
                ids.append(pid)
                if unknown:
                    bends.append(be)                                 # the whole token: tok_bend, clamped to the document
                elif key == doc[bs:be]:
                    bends.append(bs + end)                           # nothing was replaced: key bytes are source bytes
                else:
                    bends.append(source_offset(doc, bs, be, end))
            off.append(len(ids))
    return (np.array(off, np.uint64), np.array(ids, np.int32).reshape(-1), np.array(bends, np.uint32).reshape(-1), n_unknown)


# ---- the word families of both test files: (name, words, prefix, [(key, expected piece words or None for UNK)])
def _u(s):
    return s.encode()


FAMILIES = [
    ("basic", [b"[UNK]", b"un", b"##aff", b"##able"], b"##",
     [(b"unaffable", [b"un", b"##aff", b"##able"]), (b"unaffablex", None), (b"un", [b"un"]), (b"aff", None)]),
    ("no_backtracking", [b"[UNK]", b"ab", b"abc", b"##cd"], b"##", [(b"abcd", None), (b"abc", [b"abc"])]),
    ("longest_first", [b"[UNK]", b"a", b"ab", b"abc", b"##c", b"##d"], b"##", [(b"abcd", [b"abc", b"##d"]), (b"abc", [b"abc"])]),
    ("prefix_needed", [b"[UNK]", b"ab", b"cd"], b"##", [(b"abcd", None)]),
    ("prefix_given", [b"[UNK]", b"ab", b"##cd"], b"##", [(b"abcd", [b"ab", b"##cd"])]),
    ("empty_prefix", [b"[UNK]", b"ab", b"cd"], b"", [(b"abcd", [b"ab", b"cd"])]),
    ("inside_a_rune", [b"[UNK]", b"\xc3", b"##\x9f", b"Stra", b"##\xc3", b"##\x9f"], b"##", [(_u("Straß"), None)]),
    ("whole_rune", [b"[UNK]", b"\xc3", b"##\x9f", b"Stra", b"##\xc3", b"##\x9f", _u("##ß")], b"##",
     [(_u("Straß"), [b"Stra", _u("##ß")])]),
    ("replaced", [b"[UNK]", b"ab", b"##" + REPL, b"##cd", REPL], b"##",
     [(b"ab" + REPL + b"cd", [b"ab", b"##" + REPL, b"##cd"]), (REPL + REPL, [REPL, b"##" + REPL]), (b"ab" + REPL + b"x", None)]),
    ("empty_word_and_bare_prefix", [b"[UNK]", b"", b"##", b"a", b"##b"], b"##", [(b"ab", [b"a", b"##b"]), (b"ac", None), (b"", [])]),
    ("duplicates", [b"[UNK]", b"x", b"##y", b"x", b"##y", b"[UNK]"], b"##", [(b"xy", [b"x", b"##y"]), (b"xyy", [b"x", b"##y", b"##y"])]),
    ("long_prefix", [b"[UNK]", b"a", b"0123456789abcdefb"], b"0123456789abcdef", [(b"ab", [b"a", b"0123456789abcdefb"])]),
]


def family_ids(words, expected):
    """The expected piece words of a FAMILIES case as ids: the lowest index of each (None: [0], the unknown piece)."""
    return [0] if expected is None else [words.index(w) for w in expected]
