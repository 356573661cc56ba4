"""The vocabulary table on the host (dtk_vocab_probe_mem, include/datok_gpu.h), CPU tier: the builder and the probe of
datok_amd/csrc/dtk_vocab_core.h -- the code the lookup kernel runs -- against the definition of tests/tokenids.py.  The
result is exact: every comparison is an equality."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

import tokenids
from tokenids import LAST_BYTE, PREFIXES, numbered


def _probe(words, key):
    import datok_amd
    return datok_amd.Vocab.probe(words, key)


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


def _near(w):
    """A word plus one byte, minus one byte, and with its last byte changed."""
    out = [w + b"!", w + b"\x00", b"!" + w]
    if w:
        out += [w[:-1], w[1:], w[:-1] + bytes([w[-1] ^ 1])]
    return out


def _check_all(words, sample=None):
    d = tokenids.vocab_dict(words)
    for w in (words if sample is None else sample):
        assert _probe(words, w) == d[w], w
    for w in (words if sample is None else sample)[:40]:
        for k in _near(w):
            assert _probe(words, k) == d.get(k, -1), (w, k)


@pytest.mark.parametrize("bits", [-1, 0, 1, 2])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 1000])
def test_every_word_of_a_vocabulary(n, bits):
    """n_words 0, 1, 2, 3, 5 and 1000, with the whole hash and with 0, 1 and 2 bits of it (every word then shares one,
    two or four buckets and one tag): every word's own index, -1 for its neighbours."""
    words = numbered(n)
    # (a table is built per probe: under the hook 1000 words chain through one run of slots, so a sample of them)
    sample = None if n < 1000 or bits < 0 else words[::97] + words[-3:]
    with hash_bits(bits):
        _check_all(words, sample)
        assert _probe(words, b"") == -1 and _probe(words, b"w") == -1 and _probe(words, b"w%d" % n) == -1


@pytest.mark.parametrize("bits", [-1, 0, 2])
def test_prefixes_last_bytes_empty_word_and_duplicates(bits):
    words = PREFIXES + LAST_BYTE + [b"", b"\x00", b"\x00\x00", b"\xef\xbf\xbd", b"\xff", "Grüße".encode()]
    with hash_bits(bits):
        _check_all(words)
        assert _probe(words, b"") == words.index(b"")
        assert _probe(PREFIXES, b"") == -1 and _probe(PREFIXES, b"abcdef") == -1 and _probe(PREFIXES, b"abcdefg") == -1
        # duplicates: the lowest index wins, wherever the copies stand
        dup = [b"der", b"die", b"der", b"", b"das", b"die", b"", b"der"]
        for w in dup:
            assert _probe(dup, w) == dup.index(w)
        assert _probe(dup, b"de") == -1
        assert _probe([b"x"] * 9, b"x") == 0


def test_keys_that_collide_and_the_probe_wrapping_past_the_table_end():
    """Under VOCAB_HASH_BITS=2 a table has four buckets and one tag.  Words chosen with the hash's mirror: two words whose
    home is the last slot of a four-slot table (the second wraps to slot 0), an absent key of the same bucket (its probe
    walks over both, compares bytes, wraps and ends at an empty slot), and a one-word table whose word sits in slot 1."""
    cand = [b"k%d" % i for i in range(400)]
    with hash_bits(2):
        last = [k for k in cand if tokenids.home_slot(k, 2, 2) == 3]
        assert len(last) >= 3
        words = last[:2]
        assert tokenids.n_slots(2) == 4
        assert [_probe(words, w) for w in words] == [0, 1]
        assert _probe(words, last[2]) == -1                       # same bucket, same tag, other bytes
        assert _probe(list(reversed(words)), words[0]) == 1
        odd = [k for k in cand if tokenids.home_slot(k, 1, 2) == 1]
        assert _probe(odd[:1], odd[0]) == 0 and _probe(odd[:1], odd[1]) == -1
        # 1000 words in four buckets: any absent key collides with a quarter of them
        words = numbered(1000)
        assert {tokenids.hash64(w, 2) for w in words} == {0, 1, 2, 3}
        for k in (b"nicht da", b"w1000", b"W1"):
            assert _probe(words, k) == -1
    # the mirror is the library's hash: a key's home slot decides where a full-width table puts it, and the ids agree
    words = numbered(5)
    assert len({tokenids.home_slot(w, 5) for w in words}) >= 2
    assert [_probe(words, w) for w in words] == list(range(5))


def _raw_probe(blob, off, n, key=b"x"):
    import datok_amd
    L = datok_amd.lib()
    off = np.asarray(off, dtype=np.uint64)
    buf = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)
    out = C.c_int32(7)
    rc = L.dtk_vocab_probe_mem(buf.ctypes.data, off.ctypes.data, n, key, len(key), C.byref(out))
    return rc, out.value


def test_bad_offsets_are_argument_errors():
    from datok_amd import _lib
    assert _raw_probe(b"abx", [0, 2, 3], 2) == (_lib.OK, 1)
    assert _raw_probe(b"abx", [0, 3, 2], 2)[0] == _lib.E_ARG       # do not ascend
    assert _raw_probe(b"abx", [1, 2, 3], 2)[0] == _lib.E_ARG       # off[0] != 0
    assert _raw_probe(b"abx", [0, 2, 1 << 32], 2)[0] == _lib.E_ARG  # 2^32 bytes and more
    assert _raw_probe(b"", [0], 0) == (_lib.OK, -1)
    import datok_amd
    L = datok_amd.lib()
    out = C.c_int32(0)
    assert L.dtk_vocab_probe_mem(None, None, 0, b"x", 1, C.byref(out)) == _lib.E_ARG
    off = np.array([0, 1], dtype=np.uint64)
    assert L.dtk_vocab_probe_mem(None, off.ctypes.data, 1, b"x", 1, C.byref(out)) == _lib.E_ARG   # bytes missing
    assert L.dtk_vocab_probe_mem(None, off.ctypes.data, 1, b"x", 1, None) == _lib.E_ARG
    h = C.c_void_p()
    bad = np.array([0, 3, 2], dtype=np.uint64)
    buf = np.frombuffer(b"abx", dtype=np.uint8)
    assert L.dtk_vocab_create(buf.ctypes.data, bad.ctypes.data, 2, C.byref(h)) == _lib.E_ARG and not h.value


def test_create_needs_a_device_and_the_probe_does_not():
    import datok_amd
    from datok_amd import _lib
    words = [b"der", b"die", b"das"]
    assert _probe(words, b"die") == 1
    if datok_amd.lib().dtk_device_count() > 0:
        assert datok_amd.Vocab(words).size == 3
    else:
        with pytest.raises(_lib.DatokGpuError) as e:
            datok_amd.Vocab(words)
        assert e.value.code == _lib.E_NO_DEVICE


def test_the_hook_accepts_its_default_and_changes_no_result():
    import datok_amd
    L = datok_amd.lib()
    assert L.dtk_debug_configure(b"VOCAB_HASH_BITS", b"-1") == 0
    assert L.dtk_debug_configure(b"DATOK_VOCAB_HASH_BITS", b"-1") == 0
    words = PREFIXES + LAST_BYTE + numbered(50)
    keys = words + [k for w in words[:12] for k in _near(w)]
    plain = [_probe(words, k) for k in keys]
    for bits in (0, 1, 2, 7):
        with hash_bits(bits):
            assert [_probe(words, k) for k in keys] == plain, bits
    assert plain == [tokenids.lookup(words, k) for k in keys]
