"""The definition of a token's vocabulary id in plain Python (test infrastructure): tests/test_token_ids_host.py,
tests/test_token_ids.py.

A vocabulary is an ordered list of byte strings; of equal words the lowest index wins.  The key of a token is its
surface as the reference's writer prints it, string(buf[offset:]) (token_writer.go:85,93): the document's bytes
[tok_bstart, tok_bend) decoded the way Go ranges over them -- a byte that does not decode is U+FFFD of width 1, ONE
PER BYTE (Python's errors="replace" would merge a truncated sequence into one) -- and encoded again.  A row with
tok_bstart > tok_bend has no key (-1); offsets behind the document's end are clamped to it.
"""
import numpy as np

from datok_amd.host import _decode_runes, _runes_to_bytes

UNKNOWN = -1


def key_of(doc: bytes, bstart: int, bend: int):
    """The key bytes of one token row of `doc`, or None for a row the reference cannot print."""
    if bstart > bend:
        return None
    return _runes_to_bytes(_decode_runes(doc[bstart:bend]))      # (a slice clamps to the document by itself)


def vocab_dict(words):
    d = {}
    for i, w in enumerate(words):
        d.setdefault(bytes(w), i)                                # the lowest index wins
    return d


def lookup(words, key):
    return UNKNOWN if key is None else vocab_dict(words).get(bytes(key), UNKNOWN)


def keys_of_batch(text, doc_off, tok_off, tok_bstart, tok_bend):
    """The keys of every token of a batch, in the order tok_off indexes, from the arrays one run delivered."""
    raw = bytes(text)
    out = []
    for d in range(len(doc_off) - 1):
        doc = raw[int(doc_off[d]):int(doc_off[d + 1])]
        for i in range(int(tok_off[d]), int(tok_off[d + 1])):
            out.append(key_of(doc, int(tok_bstart[i]), int(tok_bend[i])))
    return out


def expected_ids(words, keys):
    d = vocab_dict(words)
    return np.array([UNKNOWN if k is None else d.get(k, UNKNOWN) for k in keys], dtype=np.int32)


def expected_counts(words, ids):
    """What a tally holds after these ids: one counter per word, the unknown ones in the last slot."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.bincount(np.where(ids < 0, len(words), ids), minlength=len(words) + 1).astype(np.uint64)


# ---- the table's hash (datok_amd/csrc/dtk_vocab_core.h), so that a test can pick words that share a bucket or sit in a
#      table's last slot instead of hoping for them.  A mirror for choosing inputs only: no expected id comes from it.
_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def hash64(key: bytes, hash_bits=-1):
    a, b = 0x811C9DC5, 0x9E3779B9
    for c in key:
        a = ((a ^ c) * 0x01000193) & _M32
        x = b ^ ((c * 0xCC9E2D51) & _M32)
        b = ((((x << 13) | (x >> 19)) & _M32) * 5 + 0xE6546B64) & _M32
    x = ((b << 32) | a) ^ ((len(key) * 0x9E3779B97F4A7C15) & _M64)
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _M64
    x ^= x >> 33
    if 0 <= hash_bits < 64:
        x &= (1 << hash_bits) - 1
    return x


def n_slots(n_words):
    n = 2
    while n < 2 * n_words:
        n *= 2
    return n


def home_slot(key: bytes, n_words, hash_bits=-1):
    return hash64(key, hash_bits) & (n_slots(n_words) - 1)


# ---- word families of both test files
PREFIXES = [b"a", b"ab", b"abc", b"abcd", b"abcde", b"abcdefgh", b"abcdefghi"]          # prefixes of one another
LAST_BYTE = [b"Wort" + bytes([c]) for c in b"abcxyz"] + [b"x" * 17 + bytes([c]) for c in b"01"]   # differ in the last byte


def numbered(n):
    return [b"w%d" % i for i in range(n)]
