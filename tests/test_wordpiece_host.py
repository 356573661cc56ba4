"""The WordPiece rule on the host (dtk_wordpiece_probe_mem, include/datok_gpu.h), CPU tier: the builder and the rule of
datok_amd/csrc/dtk_wordpiece_core.h -- the code the kernels run -- against the definition of tests/wordpiece.py, and that
definition against an independent implementation where one is installed.  The result is exact: every comparison is an
equality."""
import ctypes as C
import random
from contextlib import contextmanager

import numpy as np
import pytest

import tokenids
from wordpiece import FAMILIES, REPL, family_ids, split_key


def _probe(words, key, prefix=b"##", unk_id=0, max_runes=0, cap=None):
    import datok_amd
    ids, ends = datok_amd.wordpiece_probe(words, key, prefix=prefix, unk_id=unk_id, max_runes=max_runes, cap=cap)
    assert ids.dtype == np.int32 and ends.dtype == np.uint32
    return list(zip(ids.tolist(), ends.tolist()))


def _agree(words, key, prefix=b"##", unk_id=0, max_runes=0):
    """The probe's pieces are the definition's; returns them."""
    exp, _ = split_key(words, key, prefix, unk_id, max_runes)
    got = _probe(words, key, prefix, unk_id, max_runes)
    assert got == exp, (words, key, prefix, got, exp)
    return got


@contextmanager
def hash_bits(n):
    """The test hook VOCAB_HASH_BITS for the tables built inside the block."""
    import datok_amd
    L = datok_amd.lib()
    assert L.dtk_debug_configure(b"VOCAB_HASH_BITS", str(n).encode()) == 0
    try:
        yield
    finally:
        assert L.dtk_debug_configure(b"VOCAB_HASH_BITS", b"-1") == 0


@pytest.mark.parametrize("bits", [-1, 0, 2])
@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_families(family, bits):
    """Every family of the issue: the pieces are the stated words, and the definition says the same."""
    _, words, prefix, cases = family
    with hash_bits(bits):
        for key, expected in cases:
            got = _agree(words, key, prefix)
            assert [i for i, _ in got] == (family_ids(words, expected) if key else []), (key, got)
            if expected is None:
                assert got == [(0, len(key))]                       # the whole token, whatever was found before
            else:
                lens = [len(w) - (len(prefix) if k else 0) for k, w in enumerate(expected)]
                assert [e for _, e in got] == np.cumsum(lens).tolist()


def test_the_stated_splits():
    """The issue's tables, literally."""
    v = [b"[UNK]", b"un", b"##aff", b"##able"]
    assert _probe(v, b"unaffable") == [(1, 2), (2, 5), (3, 9)]
    assert _probe(v, b"unaffablex") == [(0, 10)]
    assert _probe([b"ab", b"abc", b"##cd"], b"abcd", unk_id=1) == [(1, 4)]            # greedy, no backtracking
    assert _probe([b"a", b"ab", b"abc", b"##c", b"##d"], b"abcd") == [(2, 3), (4, 4)]  # longest first
    assert _probe([b"ab", b"cd"], b"abcd") == [(0, 4)]                                # the prefix is not optional
    assert _probe([b"ab", b"##cd"], b"abcd") == [(0, 2), (1, 4)]
    assert _probe([b"ab", b"cd"], b"abcd", prefix=b"") == [(0, 2), (1, 4)]            # the empty prefix
    runes = [b"\xc3", b"##\x9f", b"Stra", b"##\xc3", b"##\x9f"]
    key = "Straß".encode()
    assert _probe(runes, key, unk_id=4) == [(4, 6)]                                   # no cut inside a rune
    assert _probe(runes + ["##ß".encode()], key, unk_id=4) == [(2, 4), (5, 6)]
    assert _probe([b"x", b"##" + REPL], b"x" + REPL) == [(0, 1), (1, 4)]              # a replaced byte: a piece of its own
    assert _probe(v, b"") == []                                                       # BERT returns [] here
    assert _probe([b"", b"##", b"a"], b"a", unk_id=2) == [(2, 1)]
    assert _probe([b"", b"##", b"a"], b"aa", unk_id=1) == [(1, 2)]                    # neither "" nor a bare ## matches
    assert _probe([b"x", b"##y", b"x", b"##y"], b"xy", unk_id=3) == [(0, 1), (1, 2)]  # duplicates: the lowest index


def test_max_runes_counts_runes_not_bytes():
    a = "ä".encode()
    words = [b"[UNK]", a, b"##" + a, b"a", b"##a"]
    assert _agree(words, a * 5, max_runes=5) == [(1, 2), (2, 4), (2, 6), (2, 8), (2, 10)]
    assert _agree(words, a * 6, max_runes=5) == [(0, 12)]
    assert _agree(words, a * 6, max_runes=6)[-1] == (2, 12)
    assert _agree(words, REPL * 5, max_runes=5) == [(0, 15)]        # (five runes of three bytes: split, and no word has them)
    # the default is 100
    got = _agree(words, b"a" * 100)
    assert got == [(3, 1)] + [(4, e) for e in range(2, 101)]
    assert _agree(words, b"a" * 101) == [(0, 101)]
    assert len(_agree(words, b"a" * 101, max_runes=101)) == 101
    assert _agree(words, a * 100)[-1] == (2, 200) and _agree(words, a * 101) == [(0, 202)]
    # a word of more runes than max_runes is unknown even though the vocabulary holds it
    assert _agree([b"[UNK]", b"abcdef"], b"abcdef", max_runes=5) == [(0, 6)]
    assert _agree([b"[UNK]", b"abcdef"], b"abcdef", max_runes=6) == [(1, 6)]


def test_argument_errors():
    import datok_amd
    from datok_amd import _lib
    words = [b"a", b"##b"]

    def code(**kw):
        with pytest.raises(_lib.DatokGpuError) as e:
            datok_amd.wordpiece_probe(words, b"ab", **kw)
        return e.value

    assert code(unk_id=2).code == _lib.E_ARG and code(unk_id=-1).code == _lib.E_ARG
    assert code(prefix=b"#" * 17).code == _lib.E_ARG
    assert _probe(words + [b"#" * 16 + b"b"], b"ab", prefix=b"#" * 16) == [(0, 1), (2, 2)]      # 16 bytes are allowed
    with pytest.raises(_lib.DatokGpuError) as e:
        datok_amd.wordpiece_probe([], b"ab")                        # no unk_id fits an empty vocabulary
    assert e.value.code == _lib.E_ARG
    L = datok_amd.lib()
    blob, off = np.frombuffer(b"a##b", dtype=np.uint8), np.array([0, 1, 4], dtype=np.uint64)
    ids, ends, n = np.zeros(4, np.int32), np.zeros(4, np.uint32), C.c_uint32(9)
    args = (blob.ctypes.data, off.ctypes.data, 2, b"##", 2, 0, 0, b"ab", 2)
    assert L.dtk_wordpiece_probe_mem(*args, ids.ctypes.data, ends.ctypes.data, 4, C.byref(n)) == _lib.OK and n.value == 2
    assert L.dtk_wordpiece_probe_mem(*args, ids.ctypes.data, ends.ctypes.data, 4, None) == _lib.E_ARG
    assert L.dtk_wordpiece_probe_mem(*args, None, ends.ctypes.data, 4, C.byref(n)) == _lib.E_ARG
    assert L.dtk_wordpiece_probe_mem(*args[:3], None, 2, 0, 0, b"ab", 2, ids.ctypes.data, ends.ctypes.data, 4, C.byref(n)) == _lib.E_ARG
    bad = np.array([0, 3, 2], dtype=np.uint64)
    assert L.dtk_wordpiece_probe_mem(blob.ctypes.data, bad.ctypes.data, *args[2:], ids.ctypes.data, ends.ctypes.data, 4,
                                     C.byref(n)) == _lib.E_ARG


def test_capacity():
    """cap too small: DTK_E_CAPACITY with the needed count, and the pieces that fit are there."""
    from datok_amd import _lib
    words = [b"[UNK]", b"un", b"##aff", b"##able"]
    for cap in (0, 1, 2):
        with pytest.raises(_lib.DatokGpuError) as e:
            _probe(words, b"unaffable", cap=cap)
        assert e.value.code == _lib.E_CAPACITY and e.value.needed == 3
    assert _probe(words, b"unaffable", cap=3) == [(1, 2), (2, 5), (3, 9)]
    assert _probe(words, b"unaffablex", cap=1) == [(0, 10)]         # an unknown token needs one
    with pytest.raises(_lib.DatokGpuError) as e:
        _probe(words, b"unaffablex", cap=0)
    assert e.value.code == _lib.E_CAPACITY and e.value.needed == 1
    assert _probe(words, b"", cap=0) == []


def test_continuation_words_that_collide_and_wrap():
    """Under VOCAB_HASH_BITS=2 a table has four buckets and one tag.  Words chosen with the hash's mirror: a first piece
    and a continuation word whose home is the last slot of a four-slot table, so whichever comes second wraps to slot 0;
    then three continuation words and a first piece that share one bucket of an eight-slot table -- the bytes decide, and
    an absent continuation of that bucket ends the token."""
    cand = [b"##k%d" % i for i in range(600)]
    heads = [b"h%d" % i for i in range(400)]
    with hash_bits(2):
        assert tokenids.n_slots(2) == 4 and tokenids.n_slots(4) == 8
        last = [k for k in cand if tokenids.home_slot(k, 2, 2) == 3]
        head = next(w for w in heads if tokenids.home_slot(w, 2, 2) == 3)
        key = head + last[0][2:]
        assert _agree([head, last[0]], key) == [(0, len(head)), (1, len(key))]
        assert _agree([last[0], head], key, unk_id=1) == [(1, len(head)), (0, len(key))]
        assert _agree([head, last[0]], head + last[1][2:]) == [(0, len(head) + len(last[1]) - 2)]
        same = [k for k in cand if tokenids.home_slot(k, 4, 2) == 3]
        assert len(same) >= 4
        head = next(w for w in heads if tokenids.home_slot(w, 4, 2) == 3)
        words = [head] + same[:3]
        for k, w in enumerate(same[:3]):
            assert _agree(words, head + w[2:]) == [(0, len(head)), (k + 1, len(head) + len(w) - 2)]
        assert _agree(words, head + same[3][2:]) == [(0, len(head) + len(same[3]) - 2)]
        key = head + same[2][2:] + same[0][2:] + same[1][2:]
        assert [i for i, _ in _agree(words, key)] == [0, 3, 1, 2]
        # 0 bits: every word in one bucket
    with hash_bits(0):
        words = [b"[UNK]"] + [b"w%d" % i for i in range(60)] + [b"##w%d" % i for i in range(60)]
        assert [i for i, _ in _agree(words, b"w7w59w0")] == [8, 120, 61]
        assert _agree(words, b"w7w60") == [(0, 5)]


def _random_case(rng):
    alphabet = ["a", "b", "c", "ä", "ß", "€", "\U00010330"]
    def word(lo, hi):
        return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))
    # (words of one or two letters, many of them: a fair share of the keys splits, and a fair share does not)
    words = ["[UNK]"] + sorted({word(1, 2) for _ in range(rng.randint(4, 30))}) + \
        sorted({"##" + word(1, 2) for _ in range(rng.randint(4, 40))})
    rng.shuffle(words)
    return words, [word(1, 7) for _ in range(8)]


def test_random_keys_agree_with_the_definition():
    """400 seeded random keys over a small alphabet with letters of 1 to 4 bytes, random vocabularies, max_runes 0 and 6."""
    rng = random.Random(20260401)
    split = 0
    for _ in range(50):
        words, keys = _random_case(rng)
        bw = [w.encode() for w in words]
        for key in keys:
            for max_runes in (0, 6):
                got = _agree(bw, key.encode(), unk_id=bw.index(b"[UNK]"), max_runes=max_runes)
                split += len(got) > 1
    assert split > 100


def test_the_definition_is_the_tokenizers_package_wordpiece():
    """split_key equals tokenizers.models.WordPiece(...).tokenize in ids and byte spans: the restatement pinned to an
    independent implementation (where it is installed)."""
    tokenizers = pytest.importorskip("tokenizers")
    rng = random.Random(7)
    n = split = 0
    for _ in range(50):
        words, keys = _random_case(rng)
        vocab = {w: i for i, w in enumerate(words)}
        bw = [w.encode() for w in words]
        for max_runes in (100, 6):
            model = tokenizers.models.WordPiece(vocab=vocab, unk_token="[UNK]", max_input_chars_per_word=max_runes,
                                                continuing_subword_prefix="##")
            for key in keys:
                kb = key.encode()
                exp, _ = split_key(bw, kb, b"##", vocab["[UNK]"], max_runes)
                toks = model.tokenize(key)
                assert [t.id for t in toks] == [i for i, _ in exp], (words, key)
                assert [t.offsets[1] for t in toks] == [e for _, e in exp], (words, key)
                assert [t.offsets[0] for t in toks] == ([0] + [e for _, e in exp][:-1] if toks else []), (words, key)
                n += 1
                split += len(exp) > 1
    assert n == 800 and split > 100
