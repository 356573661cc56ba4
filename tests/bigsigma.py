"""Tokenizers with more than 255 distinct symbol-stream entries, made from real ones (test infrastructure).

The symbol stream holds one-byte codes while the model's distinct entries fit a byte, else the 16-bit entries
themselves (datok_amd/csrc/dtk_model.cpp, build_images).  `tokenizer_de.matok` uses 202 of the 255 codes; a sigma
with 54 more characters beyond U+00FF does not fit any more.

enlarge_matok  appends characters to the sigma of a real `.matok`: the header's sigma count grows, the UTF-8 of the new
               characters is appended to the sigma block, and every new symbol gets a copy of the column of an existing
               character -- array[(a - 1) * stateCount + t], as wide.parse_matok reads it (matrix.go:463).  On text
               without the new characters the automaton is the original one, which the reference's goldens pin; with
               them, the expected values are the oracle's on the enlarged file.
"""
import gzip
import os
import struct

import numpy as np

import craft
import wide
from conftest import MODELS

# 64 characters from U+0400 on (two bytes each): 40 behave like "a", 12 like ".", 12 like " " -- a wrong entry for one
# of the last two groups moves token and sentence offsets, not just a symbol
CHARS = [chr(0x400 + i) for i in range(64)]
LIKE = ["a"] * 40 + ["."] * 12 + [" "] * 12
LETTERS, STOPS, BLANKS = CHARS[:40], CHARS[40:52], CHARS[52:]
# ... and for the window-edge documents a rune of three and one of four bytes, letters too
CHAR3, CHAR4 = chr(0x4E00), chr(0x1F600)
OUTSIDE = chr(0xA000)      # in no sigma here


def enlarge_matok(gz: bytes, chars, like) -> bytes:
    """The `.matok` image `gz` with `chars` appended to its sigma; chars[i] gets the arcs of the character like[i]."""
    (ver, eps, unk, ident, n, s), sig, arr = wide.parse_matok(gz)
    sigma = sig.decode("utf-8")
    assert len(sigma) == s and len(chars) == len(like)
    k = len(chars)
    out = np.zeros((n + 1) * (s + k), dtype=np.uint32)
    out[:(s - 1) * n + 1] = arr[:(s - 1) * n + 1]
    for j, (c, l) in enumerate(zip(chars, like)):
        assert c not in sigma and len(c) == 1
        al, a = sigma.rindex(l), s + j          # (a later index of the sigma block wins, like the reference's map)
        assert al > 0
        out[(a - 1) * n + 1:(a - 1) * n + n + 1] = arr[(al - 1) * n + 1:(al - 1) * n + n + 1]
    hdr = b"MATOK" + struct.pack("<HHHHIH", ver, eps, unk, ident, n, s + k)
    return gzip.compress(hdr + sig + "".join(chars).encode("utf-8") + b"M" + out.astype("<u4").tobytes(), 1)


def read_model(name):
    with open(os.path.join(MODELS, name), "rb") as f:
        return f.read()


_cache = {}


def enlarged_de(k=64, edge=False) -> bytes:
    """tokenizer_de.matok with the first k of CHARS (cached); edge: CHAR3 and CHAR4 as well."""
    key = ("de", k, edge)
    if key not in _cache:
        chars, like = CHARS[:k], LIKE[:k]
        if edge:
            chars, like = chars + [CHAR3, CHAR4], like + ["a", "a"]
        _cache[key] = enlarge_matok(read_model("tokenizer_de.matok"), chars, like)
    return _cache[key]


def oracle_of(blob):
    from oracle import oracle as O
    if id(blob) not in _cache:
        _cache[id(blob)] = (blob, O.Model(raw=gzip.decompress(blob)))
    return _cache[id(blob)][1]


# ---- device models by name, for the fixtures of the stream and batch-reader tests
# name              what is loaded
# <file>            the fixture file as it is
# <file>:pairs      ... with the hook NO_DENSE: a double array walked as pairs
# <file>:entries    ... with the hook SYM16: the stream holds the 16-bit entries, walked by the lean loop
# <file>:entries-general   ... with SYM16 and GENERAL16: 16-bit entries on the general loop
# de64.matok        enlarged_de(64): a model that has more than 255 entries by itself
_HOOKS = {"": (), "pairs": ("NO_DENSE",), "entries": ("SYM16",), "entries-general": ("SYM16", "GENERAL16")}
_LOOP_SWITCHES = ("DATOK_NO_FUSED", "DATOK_FORCE_WIDE", "DATOK_NO_DENSE", "DATOK_GENERAL16")


def has_code_twin():
    """False where the whole suite runs under DATOK_SYM16: then no load gives a stream of codes to compare with."""
    return not os.environ.get("DATOK_SYM16")


def device_model(name):
    """(device tokenizer, oracle model) of `name`.  The hooks are read at model load only (dtk_model.cpp, build_images):
    they are set around the load alone and put back to what the environment says, so that no later load in the process
    sees them -- and a suite that runs whole under one of the switches stays under it."""
    import tempfile
    import datok_amd
    from oracle import oracle as O
    fname, _, how = name.partition(":")
    configure = datok_amd.lib().dtk_debug_configure
    for hook in _HOOKS[how]:
        assert configure(hook.encode(), b"1") == 0
    try:
        if fname == "de64.matok":
            blob = enlarged_de(64)
            with tempfile.TemporaryDirectory() as where:
                path = os.path.join(where, fname)
                with open(path, "wb") as f:
                    f.write(blob)
                tok = datok_amd.load_tokenizer_file(path)
            om = oracle_of(blob)
        else:
            path = os.path.join(MODELS, fname)
            tok, om = datok_amd.load_tokenizer_file(path), O.Model(path)
    finally:
        for hook in _HOOKS[how]:
            assert configure(hook.encode(), os.environ.get("DATOK_" + hook, "0").encode()) == 0
    assert tok is not None, name
    lean = not any(os.environ.get(k) for k in _LOOP_SWITCHES)      # (those switches select the general loop)
    if how == "pairs":
        assert tok.info["dense_states"] == 0, tok.info
    elif how == "entries":
        assert tok.info["stream_codes"] == 0 and (tok.info["lean_walk"] == 1 or not lean), tok.info
    elif how == "entries-general":
        assert tok.info["stream_codes"] == 0 and tok.info["lean_walk"] == 0, tok.info
    elif fname == "de64.matok":
        assert tok.info["stream_codes"] == 0, tok.info
    return tok, om


def invalid_documents():
    """Documents for enlarged_de(64) with the new letters beside bytes that do not decode: two letters on either side of
    an \\xff; tokens that end in \\xd0, the new alphabet's lead byte, without its continuation; one letter between two
    \\xff; the first document again with a literal U+FFFD in the bad byte's place; valid text; an empty document; other
    truncated sequences beside a letter."""
    a, b, c, d, e = (x.encode() for x in LETTERS[:5])
    return [a + b + b"\xff" + c + d + b" ef", b"Preis" + a + b"\xd0 hier und " + b + b"\xd0", b"\xff" + c + b"\xff gut",
            a + b + "�".encode() + c + d + b" da", b"ganz normal", b"", b"x\xc3 " + e + b"\xf0\x9f\x98 z\x80" + e]


# The window-edge documents put an item at every document-relative position 0 .. 2 W + 1 for a row of W entries.  The
# library ships rows of 16 entries; rows of 32 are the variant it was measured against.  The tests do
# not ask the build which it is: they cover the longer one, which contains the other's positions.
EDGE_POSITIONS = 2 * 32 + 2


def splice(doc: bytes, rng, every=23, limit=None) -> bytes:
    """German text with the new characters spliced in: a letter inside a word becomes one of LETTERS, a ". " one of
    STOPS and a blank, a blank between words one of BLANKS -- about one replacement per `every` bytes.  limit: cut the
    result there, in front of a rune."""
    s = doc.decode("utf-8")
    out, i, nxt = [], 0, int(rng.integers(1, every))
    while i < len(s):
        c = s[i]
        if i >= nxt:
            kind = int(rng.integers(0, 3))
            if kind == 0 and c.isalpha() and c.islower() and i + 1 < len(s) and s[i + 1].isalpha():
                out.append(LETTERS[int(rng.integers(0, 40))]); nxt = i + int(rng.integers(1, 2 * every))
            elif kind == 1 and c == "." and i + 1 < len(s) and s[i + 1] == " ":
                out.append(STOPS[int(rng.integers(0, 12))]); nxt = i + int(rng.integers(1, 2 * every))
            elif kind == 2 and c == " " and i > 0 and s[i - 1].isalpha():
                out.append(BLANKS[int(rng.integers(0, 12))]); nxt = i + int(rng.integers(1, 2 * every))
            else:
                out.append(c)
        else:
            out.append(c)
        i += 1
    b = "".join(out).encode("utf-8")
    if limit is not None and len(b) > limit:
        b = b[:limit]
        while b and (b[-1] & 0xC0) == 0x80:
            b = b[:-1]
        if b and b[-1] >= 0xC0:
            b = b[:-1]
    return b


def german_spliced(n_docs=64, doc_bytes=4096, seed=31):
    """(text, doc_off, docs): n_docs German documents of at most doc_bytes with the new characters spliced in (cached)."""
    from datok_amd import corpus
    key = ("german", n_docs, doc_bytes, seed)
    if key not in _cache:
        text, off = corpus.german_docs(n_docs, doc_bytes, seed=seed)
        raw, rng = text.tobytes(), np.random.default_rng(seed)
        docs = [splice(raw[int(off[d]):int(off[d + 1])], rng, limit=doc_bytes) for d in range(n_docs)]
        t, o = corpus.concat_docs(docs)
        _cache[key] = (t, o, docs)
    return _cache[key]


def crafted(kind="matok", triple=False):
    """craft's automaton (the one that reaches the exact pass; triple: three SentenceEnds at one cursor) over SIGMA plus
    the 300 characters of craft.big_sigma, forty of them letters like "a".  Returns (image, the 300 characters)."""
    extra = [chr(0x4E00 + i) for i in range(300)]
    arcs = craft._automaton(triple)
    for row in arcs.values():
        if craft.A in row:
            for j in range(40):
                row[len(craft.SIGMA) + j] = row[craft.A]
    return {"matok": craft.matok_from, "datok": craft.datok_from}[kind](arcs, craft.SIGMA + extra), extra
