"""The definition of a folded key and of a split under a fold in plain Python (test infrastructure): tests/test_fold_host.py,
tests/test_fold.py.  It restates include/datok_gpu.h (dtk_fold_create) over tests/wordpiece.py and tests/tokenids.py.

A fold F is a mapping from a code point to a str of 0..4 characters; code points it does not list fold to themselves.
For a key K, valid UTF-8 (tokenids.key_of: every byte that does not decode is U+FFFD):
  the folded key F(K)    the UTF-8 of the folds of K's runes, in order
  ids                    the lowest index of the word equal to F(K), or -1
  split                  the rule of wordpiece.split_key with cuts on rune boundaries of K, the candidate F(K[start:end))
                         resp. prefix + F(K[start:end)), a candidate whose fold is empty never matching, the largest end
                         taken, max_runes counting the runes of F(K); ends are offsets in K's bytes.
"""
import numpy as np

import tokenids
import wordpiece
from wordpiece import DEFAULT_RUNES, REPL


def fold_str(mapping, s: str) -> str:
    return "".join(mapping.get(ord(c), c) for c in s)


def fold_key(mapping, key: bytes) -> bytes:
    """F(K) of a key that is valid UTF-8."""
    return fold_str(mapping, bytes(key).decode("utf-8")).encode("utf-8")


def split_key_folded(words, key, mapping, prefix=b"##", unk_id=0, max_runes=0):
    """(pieces, unknown) like wordpiece.split_key: pieces is a list of (id, end) with end an offset in KEY bytes (the
    unfolded key's)."""
    if key is None:
        return [(unk_id, 0)], True
    key = bytes(key)
    d = tokenids.vocab_dict(words)
    ends = wordpiece.rune_ends(key)
    if len(fold_key(mapping, key).decode("utf-8")) > (max_runes or DEFAULT_RUNES):
        return [(unk_id, len(key))], True
    out, start = [], 0
    while start < len(key):
        for end in reversed([e for e in ends if e > start]):
            f = fold_key(mapping, key[start:end])
            if not f:
                continue                                             # an empty fold never matches
            w = f if start == 0 else bytes(prefix) + f
            if w in d:
                out.append((d[w], end))
                start = end
                break
        else:
            return [(unk_id, len(key))], True
    return out, False


def expected_ids(words, mapping, keys):
    """tok_id of a batch under the fold, from tokenids.keys_of_batch's keys."""
    d = tokenids.vocab_dict(words)
    return np.array([-1 if k is None else d.get(fold_key(mapping, k), -1) for k in keys], dtype=np.int32)


def expected_pieces(words, mapping, text, doc_off, tok_off, tok_bstart, tok_bend, prefix=b"##", unk_id=0, max_runes=0):
    """(piece_off uint64, piece_id int32, piece_bend uint32, n_unknown) of a batch under the fold, from the arrays one
    run delivered: wordpiece.expected_pieces with the folded split."""
    raw = bytes(text)
    keys = tokenids.keys_of_batch(text, doc_off, tok_off, tok_bstart, tok_bend)
    off, ids, bends, n_unknown = [0], [], [], 0
    memo = {}
    for d in range(len(doc_off) - 1):
        doc = raw[int(doc_off[d]):int(doc_off[d + 1])]
        for i in range(int(tok_off[d]), int(tok_off[d + 1])):
            key = keys[i]
            if key not in memo:
                memo[key] = split_key_folded(words, key, mapping, prefix, unk_id, max_runes)
            pieces, unknown = memo[key]
            bs, be = int(tok_bstart[i]), min(int(tok_bend[i]), len(doc))
            bs = min(bs, be) if key is not None else bs
            n_unknown += unknown
            for pid, end in pieces:
                ids.append(pid)
                if unknown:
                    bends.append(be)
                elif key == doc[bs:be]:
                    bends.append(bs + end)
                else:
                    bends.append(wordpiece.source_offset(doc, bs, be, end))
            off.append(len(ids))
    return (np.array(off, np.uint64), np.array(ids, np.int32).reshape(-1), np.array(bends, np.uint32).reshape(-1), n_unknown)


# ---- the hand-written test mapping: case, accents, a 3 -> 9 byte growth, a 4-byte pair, one source to two targets,
#      vanishing marks
# (every character is written as chr(code point): no literal non-ASCII text, whose normal form an editor could change)
UE, ue, AE, ACUTE, DIAERESIS = chr(0xDC), chr(0xFC), chr(0xC4), chr(0x301), chr(0x308)
HANGUL = chr(0xD55C)                              # three bytes; its jamo are nine
JAMO = chr(0x1112) + chr(0x1161) + chr(0x11AB)
DESERET, deseret = chr(0x10400), chr(0x10428)     # a pair of four bytes each
KA, O, E, AA = chr(0x995), chr(0x9CB), chr(0x9C7), chr(0x9BE)   # Bengali: O folds to E AA
HAND = {ord(c): c.lower() for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZ"}
HAND.update({0xC4: "a", 0xD6: "o", 0xDC: "u", 0xE4: "a", 0xF6: "o", 0xFC: "u", 0xC9: "e", 0xE9: "e",
             0xD55C: JAMO, 0x10400: deseret, 0x09CB: E + AA, 0x0301: "", 0x0308: ""})
HAND_REPL_VANISHES = dict(HAND)
HAND_REPL_VANISHES[0xFFFD] = ""

VANISH_WORDS = [b"[UNK]", b"", b"##", b"a", b"##b"]


def _u(s):
    return s.encode("utf-8")


_LONG = "a" * 50 + ACUTE + "a" * 49 + DIAERESIS   # 101 source runes, 99 of them stay

# (name, mapping, words, prefix, [(key, expected [(word, or None for unk_id; end in key bytes)])])
FAMILIES = [
    ("case", HAND, [b"[UNK]", b"uber"], b"##",
     [(_u(UE + "ber"), [(b"uber", 5)]), (_u(ue + "ber"), [(b"uber", 5)]), (b"UBER", [(b"uber", 4)]), (_u(UE + "bel"), [(None, 5)])]),
    ("shrink_max_word", HAND, [b"[UNK]", b"aaaa"], b"##",
     [(_u(AE * 4), [(b"aaaa", 8)]), (_u(AE * 5), [(None, 10)])]),
    ("growth_short_words", HAND, [b"[UNK]", b"ab", b"##c", _u(JAMO[0])], b"##",
     [(_u(HANGUL), [(None, 3)]), (_u("ab" + HANGUL), [(None, 5)])]),
    ("growth_jamo_word", HAND, [b"[UNK]", _u(JAMO), b"ab", _u("##" + JAMO)], b"##",
     [(_u(HANGUL), [(_u(JAMO), 3)]), (_u("ab" + HANGUL), [(b"ab", 2), (_u("##" + JAMO), 5)])]),
    ("four_byte_pair", HAND, [b"[UNK]", _u(deseret), _u("##" + deseret)], b"##",
     [(_u(DESERET), [(_u(deseret), 4)]), (_u(DESERET + deseret), [(_u(deseret), 4), (_u("##" + deseret), 8)])]),
    # (no cut lies inside the two targets of one source)
    ("one_to_two", HAND, [b"[UNK]", _u(KA + E + AA), _u(KA), _u(E), _u("##" + E), _u("##" + AA)], b"##",
     [(_u(KA + O), [(_u(KA + E + AA), 6)]), (_u(KA + KA + O), [(None, 9)]), (_u(O), [(None, 3)])]),
    ("vanishing", HAND, VANISH_WORDS, b"##",
     [(_u("a" + ACUTE + "b"), [(b"a", 3), (b"##b", 4)]), (_u("a" + ACUTE), [(b"a", 3)]), (_u(ACUTE + "a"), [(b"a", 3)]),
      (_u(ACUTE), [(None, 2)]), (_u("a" + ACUTE + DIAERESIS + "b" + ACUTE), [(b"a", 5), (b"##b", 8)]),
      (_u(ACUTE + DIAERESIS), [(None, 4)]), (_u(AE + "b"), [(b"a", 2), (b"##b", 3)]), (_u("ab" + ACUTE + "c"), [(None, 5)])]),
    ("replaced_vanishes", HAND_REPL_VANISHES, [b"[UNK]", b"ab", b"##cd"], b"##", [(b"ab" + REPL + b"cd", [(b"ab", 5), (b"##cd", 7)])]),
    ("replaced_stays", HAND, [b"[UNK]", b"ab", b"##cd", b"##" + REPL], b"##",
     [(b"AB" + REPL + b"cd", [(b"ab", 2), (b"##" + REPL, 5), (b"##cd", 7)])]),
    ("duplicate_word", HAND, [b"[UNK]", b"x", b"##y", b"x", b"##y"], b"##", [(b"XY", [(b"x", 1), (b"##y", 2)])]),
    ("prefix_state", HAND, [b"[UNK]", b"ab", b"##ab", b"cd"], b"##", [(b"ABAB", [(b"ab", 2), (b"##ab", 4)]), (b"ABCD", [(None, 4)])]),
    ("max_runes", HAND, [b"[UNK]", b"a", b"##a"], b"##",
     [(_u(_LONG), [(b"a", 1)] + [(b"##a", e) for e in range(2, 50)] + [(b"##a", 52)] + [(b"##a", e) for e in range(53, 101)] +
       [(b"##a", 103)]),
      (b"A" * 101, [(None, 101)])]),
]


def family_pieces(words, expected, unk_id=0):
    """A FAMILIES case's expectation as [(id, end)]: the lowest index of each word, unk_id for None."""
    return [(unk_id if w is None else words.index(w), e) for w, e in expected]
