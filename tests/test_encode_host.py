"""The encoding rule on the host (dtk_encode_rows_mem, include/datok_gpu.h), CPU tier: the code of dtk_encode_core.h,
which the kernels of dtk_encode.hip run too, against the plain restatement of tests/encode.py -- and that restatement
against the `tokenizers` package's truncation with stride.  Everything is exact."""
import ctypes as C
import itertools

import numpy as np
import pytest

import encode
from encode import Spec

SPECIALS = {"both": (2, 3), "cls": (2, -1), "sep": (-1, 3), "neither": (-1, -1)}


def _batch(ns, tokens=(1, 0, 2, 5)):
    """Units of ns[i] pieces each, made of tokens of 1, 0, 2, 5, 1, ... pieces (the last one cut to fit), so a unit of
    three pieces and more has a token without a piece in its middle; a unit of no piece has no token (even i) or one
    token without a piece (odd i).  Three units share a document: one begins it, two do not.  Returns (piece_off,
    piece_id, unit_tok_end, tok_off, units) with units as tests/encode.py takes them."""
    piece_off, ends, tok_off, units = [0], [], [0], []
    for i, n in enumerate(ns):
        if i % 3 == 0 and i:
            tok_off.append(len(piece_off) - 1)
        t0, left, k = len(piece_off) - 1, n, 0
        if n == 0 and i % 2:
            piece_off.append(piece_off[-1])
        while left:
            c = min(tokens[k % len(tokens)], left)
            piece_off.append(piece_off[-1] + c)
            left -= c
            k += 1
        ends.append(len(piece_off) - 1)
        units.append((t0, ends[-1], tok_off[-1]))
    tok_off.append(len(piece_off) - 1)
    piece_id = 100 + np.arange(piece_off[-1], dtype=np.int32)
    return np.array(piece_off, np.uint64), piece_id, np.array(ends, np.uint64), np.array(tok_off, np.uint64), units


def _grid():
    for (name, (cls_id, sep_id)), first_window in itertools.product(SPECIALS.items(), (False, True)):
        n_special = (cls_id >= 0) + (sep_id >= 0)
        for max_len in sorted({1 + n_special, 4, 5, 8}):
            body = max_len - n_special
            for stride in range(body):
                yield name, cls_id, sep_id, max_len, stride, first_window


def test_rows_equal_the_restatement_over_the_grid():
    """n in 0..3 * body, every stride, max_len in {1 + n_special, 4, 5, 8}, the four choices of specials, with and
    without FIRST_WINDOW and word_id."""
    import datok_amd
    checked = 0
    for name, cls_id, sep_id, max_len, stride, first_window in _grid():
        body = max_len - (cls_id >= 0) - (sep_id >= 0)
        piece_off, piece_id, ends, tok_off, units = _batch(list(range(3 * body + 1)) + [0, 0, body + 1])
        for word_ids in (False, True):
            spec = Spec(max_len, cls_id, sep_id, 1, stride, first_window, word_ids)
            got = datok_amd.encode_rows(piece_off, piece_id, ends, tok_off=tok_off if word_ids else None, **spec.kw())
            encode.assert_equal(got, encode.expected(spec, units, piece_off, piece_id), (name, max_len, stride, first_window, word_ids))
            checked += got.n_rows
    assert checked > 8000                                              # (the grid is not empty)


def test_word_ids_of_split_tokens():
    """Tokens of 1, 2 and 5 pieces and one of none in the middle of a unit; the second unit does not begin its document."""
    import datok_amd
    piece_off = np.array([0, 1, 3, 3, 8, 9, 10], np.uint64)            # tokens of 1, 2, 0, 5, 1, 1 pieces
    piece_id = np.arange(10, 20, dtype=np.int32)
    got = datok_amd.encode_rows(piece_off, piece_id, [4, 6], 8, 1, 2, 0, stride=2, word_ids=True, tok_off=[0, 6])
    assert got.unit_row_off.tolist() == [0, 2, 3] and got.n_cut == 1
    assert got.input_ids.tolist() == [[1, 10, 11, 12, 13, 14, 15, 2], [1, 14, 15, 16, 17, 2, 0, 0], [1, 18, 19, 2, 0, 0, 0, 0]]
    assert got.word_id.tolist() == [[-1, 0, 1, 1, 3, 3, 3, -1], [-1, 3, 3, 3, 3, -1, -1, -1], [-1, 4, 5, -1, -1, -1, -1, -1]]
    assert got.row_len.tolist() == [8, 6, 4] and got.row_piece0.tolist() == [0, 4, 8]
    assert got.attention_mask().tolist() == [[1] * 8, [1] * 6 + [0] * 2, [1] * 4 + [0] * 4]
    # the same pieces in two documents: the second unit begins one, and its word ids count from it
    got = datok_amd.encode_rows(piece_off, piece_id, [4, 6], 8, 1, 2, 0, stride=2, word_ids=True, tok_off=[0, 4, 6])
    assert got.word_id[2].tolist() == [-1, 0, 1, -1, -1, -1, -1, -1]
    # a unit of no piece is the row of the specials alone
    got = datok_amd.encode_rows([0, 0], [], [0, 1, 1], 4, 7, 8, 9, word_ids=True, tok_off=[0, 1])
    assert got.input_ids.tolist() == [[7, 8, 9, 9]] * 3 and got.row_len.tolist() == [2] * 3 and (got.word_id == -1).all()


def _raw(spec, piece_off, piece_id, ends, cap, n_rows, out=None, tok_off=None):
    import datok_amd
    piece_off = np.ascontiguousarray(piece_off, np.uint64)
    piece_id = np.ascontiguousarray(piece_id, np.int32)
    ends = np.ascontiguousarray(ends, np.uint64)
    off = np.zeros(len(ends) + 1, np.uint64)
    ml = max(int(spec.max_len), 1) if spec is not None else 1
    ids, rl, p0 = np.zeros(max(cap, 1) * ml, np.int32), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64)
    words = np.zeros(max(cap, 1) * ml, np.int32)
    toff = None if tok_off is None else np.ascontiguousarray(tok_off, np.uint64)
    rc = datok_amd.lib().dtk_encode_rows_mem(
        C.byref(spec) if spec is not None else None, piece_off.ctypes.data, len(piece_off) - 1, piece_id.ctypes.data,
        ends.ctypes.data, len(ends), toff.ctypes.data if toff is not None else None, 0 if toff is None else len(toff) - 1,
        cap, off.ctypes.data, ids.ctypes.data, rl.ctypes.data, p0.ctypes.data, words.ctypes.data,
        C.byref(n_rows) if n_rows is not None else None, None)
    if out is not None:
        out.update(ids=ids, off=off)
    return rc


def test_argument_checks():
    from datok_amd import _lib
    S = _lib.EncodeSpec
    piece_off, piece_id, ends = [0, 2, 3], [5, 6, 7], [2]
    n = C.c_uint64(0)
    good = dict(max_len=4, cls_id=1, sep_id=2, pad_id=0, unit=_lib.ENC_DOCUMENT, stride=1, flags=0)
    assert _raw(S(**good), piece_off, piece_id, ends, 4, n) == _lib.OK and n.value == 2
    bad = [dict(max_len=2), dict(max_len=1, sep_id=-1), dict(max_len=0, cls_id=-1, sep_id=-1),          # body >= 1
           dict(stride=2), dict(stride=3, sep_id=-1), dict(stride=0xFFFFFFFF),                          # 0 <= stride < body
           dict(max_len=65536), dict(unit=2), dict(flags=4), dict(flags=0x80000001),
           dict(cls_id=-2), dict(sep_id=-2), dict(pad_id=-1)]
    for change in bad:
        assert _raw(S(**dict(good, **change)), piece_off, piece_id, ends, 4, n) == _lib.E_ARG, change
    for ok in (dict(max_len=65535), dict(max_len=3, stride=0), dict(stride=0), dict(unit=_lib.ENC_SENTENCE), dict(flags=1),
               dict(cls_id=-1, sep_id=-1, stride=3), dict(cls_id=0, sep_id=0, pad_id=0x7FFFFFFF)):
        assert _raw(S(**dict(good, **ok)), piece_off, piece_id, ends, 4, n) == _lib.OK, ok
    assert _raw(None, piece_off, piece_id, ends, 4, n) == _lib.E_ARG
    assert _raw(S(**good), piece_off, piece_id, ends, 4, None) == _lib.E_ARG
    assert _raw(S(**good), piece_off, piece_id, [3], 4, n) == _lib.E_ARG                                  # a unit past the tokens
    assert _raw(S(**good), [0, 2, 3, 4], [5, 6, 7, 8], [2, 1], 4, n) == _lib.E_ARG                        # units descend
    assert _raw(S(**good), [0, 2, 1], piece_id, ends, 4, n) == _lib.E_ARG                                 # piece_off descends
    assert _raw(S(**dict(good, flags=2)), piece_off, piece_id, ends, 4, n) == _lib.E_ARG                  # word_id needs tok_off
    assert _raw(S(**dict(good, flags=2)), piece_off, piece_id, ends, 4, n, tok_off=[0, 1]) == _lib.E_ARG  # ... of all tokens
    assert _raw(S(**dict(good, flags=2)), piece_off, piece_id, ends, 4, n, tok_off=[0, 2]) == _lib.OK


def test_capacity_says_what_is_needed():
    import datok_amd
    from datok_amd import _lib
    piece_off, piece_id = np.arange(0, 11, dtype=np.uint64), np.arange(10, dtype=np.int32)
    spec = _lib.EncodeSpec(max_len=4, cls_id=1, sep_id=2, pad_id=0, unit=_lib.ENC_DOCUMENT, stride=1, flags=0)
    n, out = C.c_uint64(0), {}
    assert _raw(spec, piece_off, piece_id, [10, 10], 3, n, out) == _lib.E_CAPACITY and n.value == 10      # 1 + 8 rows, and 1
    assert out["off"].tolist() == [0, 9, 10]
    assert out["ids"][:12].tolist() == [1, 0, 1, 2, 1, 1, 2, 2, 1, 2, 3, 2] and not out["ids"][12:].any()  # nothing behind cap_rows
    assert _raw(spec, piece_off, piece_id, [10, 10], 10, n, out) == _lib.OK and n.value == 10
    assert _raw(spec, piece_off, piece_id, [10, 10], 0, n) == _lib.E_CAPACITY and n.value == 10
    with pytest.raises(_lib.DatokGpuError) as e:
        datok_amd.encode_rows(piece_off, piece_id, [10, 10], 4, 1, 2, 0, stride=1, cap_rows=9)
    assert e.value.code == _lib.E_CAPACITY and e.value.needed == 10
    assert datok_amd.encode_rows(piece_off, piece_id, [10, 10], 4, 1, 2, 0, stride=1).n_rows == 10


def test_restatement_against_the_tokenizers_package():
    """tests/encode.py pinned to `tokenizers`: enable_truncation(max_length, stride) with padding and a [CLS] $A [SEP]
    template on pre-tokenized input -- ids, attention mask, window contents and word ids of the first encoding followed
    by .overflowing, with a word of three pieces that window edges cut, and the input of no word."""
    tokenizers = pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer, models, processors
    vocab = {"[PAD]": 0, "[UNK]": 1, "[CLS]": 2, "[SEP]": 3}
    for i in range(40):
        vocab["w%d" % i] = 4 + i
    vocab.update({"ab": 50, "##cd": 51, "##e": 52})
    tk = Tokenizer(models.WordPiece(vocab, unk_token="[UNK]", continuing_subword_prefix="##", max_input_chars_per_word=100))
    tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 2), ("[SEP]", 3)])
    cut_inside_a_word = 0
    for n, max_len, stride in itertools.product(range(0, 30), [3, 4, 5, 8, 16], [0, 1, 2, 5]):
        if stride >= max_len - 2:
            continue
        words = ["w%d" % (i % 40) for i in range(n)]
        if n >= 3:
            words[2] = "abcde"
        tk.enable_truncation(max_length=max_len, stride=stride)
        tk.enable_padding(length=max_len, pad_id=0, pad_token="[PAD]")
        e = tk.encode(words, is_pretokenized=True)
        rows = [e] + e.overflowing
        piece_off, piece_id = [0], []
        for w in words:
            piece_id += [50, 51, 52] if w == "abcde" else [vocab[w]]
            piece_off.append(len(piece_id))
        spec = Spec(max_len, 2, 3, 0, stride, word_ids=True)
        exp = encode.expected(spec, [(0, n, 0)], np.array(piece_off, np.uint64), np.array(piece_id, np.int32))
        assert exp["n_rows"] == len(rows), (n, max_len, stride)
        assert exp["input_ids"].tolist() == [r.ids for r in rows], (n, max_len, stride)
        mask = (np.arange(max_len)[None, :] < exp["row_len"][:, None]).astype(int)
        assert mask.tolist() == [r.attention_mask for r in rows], (n, max_len, stride)
        assert exp["word_id"].tolist() == [[-1 if w is None else w for w in r.word_ids] for r in rows], (n, max_len, stride)
        for k, r in enumerate(rows):
            a = int(exp["row_piece0"][k])
            body = [i for i, m, s in zip(r.ids, r.attention_mask, r.special_tokens_mask) if m and not s]
            assert body == piece_id[a:a + len(body)]
            cut_inside_a_word += n >= 3 and 2 < a < 5
    assert cut_inside_a_word > 20
