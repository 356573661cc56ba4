"""Folded keys on the host (dtk_fold_apply_mem, dtk_wordpiece_probe_fold_mem of include/datok_gpu.h), CPU tier: the tables
and the rule of datok_amd/csrc/dtk_fold_core.h and dtk_wordpiece_core.h -- the code the kernels run -- against the
definition of tests/fold.py, and bert_uncased_mapping against an independent implementation where one is installed.
The result is exact: every comparison is an equality."""
import ctypes as C
import random

import numpy as np
import pytest

import fold
import wordpiece
from fold import ACUTE, AE, DIAERESIS, FAMILIES, HAND, HAND_REPL_VANISHES, HANGUL, JAMO, UE, family_pieces, fold_key, split_key_folded
from test_wordpiece_host import hash_bits
from wordpiece import REPL


def _probe(words, key, mapping, prefix=b"##", unk_id=0, max_runes=0, cap=None):
    import datok_amd
    ids, ends = datok_amd.wordpiece_probe(words, key, prefix=prefix, unk_id=unk_id, max_runes=max_runes, cap=cap, fold=mapping)
    assert ids.dtype == np.int32 and ends.dtype == np.uint32
    return list(zip(ids.tolist(), ends.tolist()))


def _agree(words, key, mapping, prefix=b"##", unk_id=0, max_runes=0):
    """The probe's pieces are the definition's; returns them."""
    exp, _ = split_key_folded(words, key, mapping, prefix, unk_id, max_runes)
    got = _probe(words, key, mapping, prefix, unk_id, max_runes)
    assert got == exp, (words, key, prefix, got, exp)
    return got


@pytest.mark.parametrize("bits", [-1, 0])
@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_families(family, bits):
    """Every family of tests/fold.py: the probe gives the stated pieces with ends in the bytes of the given key, the
    definition says the same, and dtk_fold_apply_mem gives the definition's folded key."""
    import datok_amd
    _, mapping, words, prefix, cases = family
    with hash_bits(bits):
        for key, expected in cases:
            assert _agree(words, key, mapping, prefix) == family_pieces(words, expected), key
            assert datok_amd.fold_apply(mapping, key) == fold_key(mapping, key)


def test_the_stated_cases():
    """The issue's list, literally."""
    u = fold._u
    assert _probe([b"[UNK]", b"uber"], u(UE + "ber"), HAND) == [(1, 5)]
    assert _probe([b"[UNK]", b"aaaa"], u(AE * 4), HAND) == [(1, 8)]              # 8 source bytes, max_word 4
    assert _probe([b"[UNK]", b"ab"], u(HANGUL), HAND) == [(0, 3)]               # 3 bytes fold to 9: rejected by length
    assert _probe([b"[UNK]", u(JAMO)], u(HANGUL), HAND) == [(1, 3)]
    assert _probe([b"[UNK]", u(fold.deseret)], u(fold.DESERET), HAND) == [(1, 4)]
    assert _probe([b"[UNK]", u(fold.KA + fold.E + fold.AA)], u(fold.KA + fold.O), HAND) == [(1, 6)]
    v = fold.VANISH_WORDS
    assert _probe(v, u("a" + ACUTE + "b"), HAND) == [(3, 3), (4, 4)]
    assert _probe(v, u("a" + ACUTE), HAND) == [(3, 3)]
    assert _probe(v, u(ACUTE + "a"), HAND) == [(3, 3)]
    assert _probe(v, u(ACUTE), HAND) == [(0, 2)]                               # neither "" nor the bare prefix matches
    assert _probe([b"[UNK]", b"ab", b"##cd"], b"ab" + REPL + b"cd", HAND_REPL_VANISHES) == [(1, 5), (2, 7)]
    assert _probe([b"[UNK]", b"x", b"##y", b"x", b"##y"], b"XY", HAND) == [(1, 1), (2, 2)]
    words = [b"[UNK]", b"a", b"##a"]
    assert len(_agree(words, u(fold._LONG), HAND)) == 99                       # 101 source runes, two of them vanish
    assert _agree(words, b"a" * 101, HAND) == [(0, 101)]                       # 101 that all stay
    assert _agree(words, u(fold._LONG), HAND, max_runes=98) == [(0, 103)]
    assert _probe(words, b"", HAND) == []


def test_the_empty_mapping_is_the_unfolded_probe():
    """Identity: with the empty mapping every FAMILIES case of tests/wordpiece.py splits as dtk_wordpiece_probe_mem does."""
    import datok_amd
    for _, words, prefix, cases in wordpiece.FAMILIES:
        for key, _ in cases:
            ids, ends = datok_amd.wordpiece_probe(words, key, prefix=prefix)
            assert _probe(words, key, {}, prefix) == list(zip(ids.tolist(), ends.tolist())), key
            assert datok_amd.fold_apply({}, key) == key


def test_apply_replaces_what_does_not_decode():
    """dtk_fold_apply_mem takes any bytes: one that does not decode is U+FFFD, one per byte, and folds as U+FFFD does."""
    import datok_amd
    import tokenids
    keys = [b"ab\xffcd", b"\xe2\x82", b"x\xc3", b"\xf0\x9f\x98 z\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
            REPL, b"A\xd0", fold._u(UE) + b"\xff"]
    for key in keys:
        k = tokenids.key_of(key, 0, len(key))
        assert datok_amd.fold_apply(HAND, key) == fold_key(HAND, k), key
        assert datok_amd.fold_apply(HAND_REPL_VANISHES, key) == fold_key(HAND_REPL_VANISHES, k), key
    assert datok_amd.fold_apply(HAND_REPL_VANISHES, b"ab\xffcd") == b"abcd"
    assert datok_amd.fold_apply(HAND, b"") == b""


def _random_case(rng):
    alphabet = ["a", "b", "A", "B", AE, UE, ACUTE, DIAERESIS, HANGUL, fold.DESERET, fold.O, chr(0x20AC)]
    folded = ["a", "b", "u", JAMO, fold.deseret, fold.E + fold.AA, fold.E, chr(0x20AC)]

    def word(lo, hi):
        return "".join(rng.choice(folded) for _ in range(rng.randint(lo, hi)))
    words = ["[UNK]"] + sorted({word(1, 2) for _ in range(rng.randint(4, 30))}) + \
        sorted({"##" + word(1, 2) for _ in range(rng.randint(4, 40))})
    rng.shuffle(words)
    return words, ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 7))) for _ in range(8)]


def test_random_keys_agree_with_the_definition():
    """800 seeded random keys whose letters shrink, grow, vanish and double under the fold, over random vocabularies in
    folded form, max_runes 0 and 6; a fair share of them splits."""
    rng = random.Random(20261021)
    split = unknown = 0
    for _ in range(50):
        words, keys = _random_case(rng)
        bw = [w.encode() for w in words]
        for key in keys:
            for max_runes in (0, 6):
                got = _agree(bw, key.encode(), HAND, unk_id=bw.index(b"[UNK]"), max_runes=max_runes)
                split += len(got) > 1
                unknown += got == [(bw.index(b"[UNK]"), len(key.encode()))]
    assert split > 100 and unknown > 100


def test_argument_errors():
    import datok_amd
    from datok_amd import _lib

    def code(mapping):
        with pytest.raises(_lib.DatokGpuError) as e:
            datok_amd.fold_apply(mapping, b"ab")
        return e.value.code
    assert code({0xD800: "a"}) == _lib.E_ARG                        # a surrogate source
    assert code({0x110000: "a"}) == _lib.E_ARG
    assert code({0x41: [0x61] * 5}) == _lib.E_ARG                   # 5 targets
    assert datok_amd.fold_apply({0x61: [0x62] * 4}, b"ab") == b"bbbbb"
    assert code({0x41: [0x110000]}) == _lib.E_ARG                   # a target above U+10FFFF
    assert code({0x41: [0xDFFF]}) == _lib.E_ARG                     # a target that is no scalar value
    L = datok_amd.lib()
    out, n = np.zeros(16, np.uint8), C.c_size_t(0)

    def raw(frm, to_off, to, key=b"ab", cap=16, n_out=n):
        frm, to_off, to = np.array(frm, np.uint32), np.array(to_off, np.uint32), np.array(to, np.uint32)
        return L.dtk_fold_apply_mem(frm.ctypes.data, to_off.ctypes.data, to.ctypes.data, len(frm), key, len(key),
                                    out.ctypes.data, cap, C.byref(n_out) if n_out is not None else None)
    assert raw([0x61, 0x62], [0, 1, 2], [0x78, 0x79]) == _lib.OK and n.value == 2 and bytes(out[:2]) == b"xy"
    assert raw([0x61, 0x61], [0, 1, 2], [0x78, 0x79]) == _lib.E_ARG            # a duplicate source
    assert raw([0x61, 0x62], [1, 1, 2], [0x78, 0x79]) == _lib.E_ARG            # to_off does not begin at 0
    assert raw([0x61, 0x62], [0, 2, 1], [0x78, 0x79]) == _lib.E_ARG            # ... or does not ascend
    assert raw([0x61, 0x62], [0, 1, 2], [0x78, 0x79], n_out=None) == _lib.E_ARG
    assert raw([0x61], [0, 3], [0x78, 0x79, 0x7A], cap=2) == _lib.E_CAPACITY and n.value == 4
    # the probe under a fold takes K, which is valid UTF-8, and checks the fold like dtk_fold_apply_mem
    for bad in (b"a\xff", b"\x80", b"\xe2\x82"):
        with pytest.raises(_lib.DatokGpuError) as e:
            datok_amd.wordpiece_probe([b"a"], bad, fold=HAND)
        assert e.value.code == _lib.E_ARG
    for mapping in ({0xD800: "a"}, {0x41: [0x61] * 5}):
        with pytest.raises(_lib.DatokGpuError) as e:
            datok_amd.wordpiece_probe([b"a"], b"a", fold=mapping)
        assert e.value.code == _lib.E_ARG
    with pytest.raises(_lib.DatokGpuError) as e:
        datok_amd.wordpiece_probe([b"a", b"##b"], b"AB", fold=HAND, cap=1)
    assert e.value.code == _lib.E_CAPACITY and e.value.needed == 2


def test_bert_uncased_mapping_properties():
    """No count that depends on the Unicode version: every source and target is a scalar value, no fold is longer than
    DTK_FOLD_MAX, no source folds to itself; and the letters everybody knows."""
    import unicodedata
    import datok_amd
    m = datok_amd.bert_uncased_mapping()
    assert m is datok_amd.bert_uncased_mapping()                    # cached
    assert all(0 <= cp <= 0x10FFFF and not 0xD800 <= cp <= 0xDFFF for cp in m)
    assert max(len(t) for t in m.values()) <= 4
    assert all(t != chr(cp) for cp, t in m.items())
    assert all(unicodedata.category(c) != "Mn" for t in m.values() for c in t)
    assert m[ord("A")] == "a" and m[0xDC] == "u" and m[0xE4] == "a" and m[0x301] == "" and m[0xD55C] == JAMO
    assert 0xDF not in m and ord("a") not in m                      # sharp s and lower-case ASCII stay
    assert m[0x3A3] == chr(0x3C3) and 0x3C2 not in m                # per rune: a final sigma is not made, and stays
    assert datok_amd.fold_apply(m, fold._u(UE + "ber " + AE + "RGER")) == b"uber arger"
    # the whole table goes through the library's tables and comes back
    sample = "".join(chr(cp) for cp in list(m)[::7])
    assert datok_amd.fold_apply(m, sample.encode()) == fold_key(m, sample.encode())


def test_bert_uncased_mapping_is_the_tokenizers_package_normalizer():
    """For every assigned code point of U+0000-U+058F, U+1E00-U+1FFF and U+AC00-U+D7A3 the fold is what
    tokenizers.normalizers.BertNormalizer(strip_accents, lowercase) makes of that character (where it is installed)."""
    tokenizers = pytest.importorskip("tokenizers")
    import unicodedata
    import datok_amd
    m = datok_amd.bert_uncased_mapping()
    norm = tokenizers.normalizers.BertNormalizer(clean_text=False, handle_chinese_chars=False, strip_accents=True, lowercase=True)
    n = 0
    for lo, hi in ((0x0000, 0x058F), (0x1E00, 0x1FFF), (0xAC00, 0xD7A3)):
        for cp in range(lo, hi + 1):
            c = chr(cp)
            if unicodedata.category(c) == "Cn":
                continue
            assert m.get(cp, c) == norm.normalize_str(c), hex(cp)
            n += 1
    assert n > 12000
