"""What tests/test_symbolize.py shares with the child process that runs its device-resident cases.

torch brings a HIP runtime of its own and can open the device only if that one is loaded before the library's (the
order bench.py has).  In the test process the library came first, so the cases that build their input from torch
tensors run in a fresh child: `python tests/symgpu.py CASE ARG ...`, which initialises torch before it loads the
library and prints DEVICE OK when every assertion held."""
import gzip
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import craft
import symref
from parity import assert_batch_equals_oracle

SIMPLE = 3
ST_EMPTY_TEXT = 2
SHIPPED = ["tokenizer_de.matok", "tokenizer_de.datok"]     # one-byte codes, sigma in LDS
CRAFTED = "crafted"                                        # 16-bit entries, sigma searched in memory
ARRAYS = ("tok_off", "sent_off", "text_off", "tok_rstart", "tok_rend", "tok_bstart", "tok_bend", "sent",
          "text_tok_end", "text_sent_end", "status", "doc_tail")


class MemoOracle:
    """The oracle, asked once per distinct document (the rows share their words)."""

    def __init__(self, om):
        self.om, self._doc, self._out = om, {}, {}

    def transduce_doc(self, doc, flags=0):
        key = (doc, flags)
        if key not in self._doc:
            self._doc[key] = self.om.transduce_doc(doc, flags)
        return self._doc[key]

    def transduce(self, doc, flags=SIMPLE):
        key = (doc, flags)
        if key not in self._out:
            self._out[key] = self.om.transduce(doc, flags)
        return self._out[key]


class Ctx:
    """name -> (device tokenizer, oracle model, memoised oracle, extra sequences of that model's corpus), the corpus
    rows, and reference streams computed once per (model, batch).  tmp_dir: where the crafted model's file goes."""

    def __init__(self, tmp_dir):
        import datok_amd
        assert datok_amd.lib().dtk_device_count() > 0, "no HIP device: the product path has no CPU fallback"
        self.tmp_dir, self._models, self._refs, self._rows = str(tmp_dir), {}, {}, {}

    def model(self, name):
        import datok_amd
        from oracle import oracle as O
        if name not in self._models:
            if name == CRAFTED:
                blob, extra = craft.big_sigma("matok")
                path = os.path.join(self.tmp_dir, "big.matok")
                with open(path, "wb") as f:
                    f.write(blob)
                tok, om = datok_amd.load_tokenizer_file(path), O.Model(raw=gzip.decompress(blob))
                more = tuple(extra[k].encode() for k in (0, 39, 40, 299))   # letters like "a", and plain members
            else:
                path = os.path.join(MODELS, name)
                tok, om, more = datok_amd.load_tokenizer_file(path), O.Model(path), ()
            assert tok is not None
            if not os.environ.get("DATOK_SYM16"):
                assert (tok.info["stream_codes"] == 0) == (name == CRAFTED), tok.info
            self._models[name] = (tok, om, MemoOracle(om), more)
        return self._models[name]

    def rows(self, name):
        more = self.model(name)[3]
        if more not in self._rows:
            self._rows[more] = symref.rows(more)
        return self._rows[more]

    def ref(self, name, key, text, off):
        """reference_stream of a batch, kept under (model, key)."""
        if (name, key) not in self._refs:
            self._refs[(name, key)] = symref.reference_stream(self.model(name)[1], text, off)
        return self._refs[(name, key)]


def run_batch(tok, text, off, max_bytes=None, max_docs=None):
    import datok_amd
    b = datok_amd.Batch(max(len(text), 1) if max_bytes is None else max_bytes, (len(off) - 1) if max_docs is None else max_docs)
    b.set_input(text, off)
    b.run(tok, 0)
    return b


def rows_batch(ctx, name, lay):
    """(key, text, doc_off) of a layout of the rows; "c@N": layout (c) of the text from byte N on."""
    text, what = ctx.rows(name)
    if "@" in lay:
        first = {"8192": 8192, "row1": symref.ROW + 8192 - 1}[lay.split("@")[1]]
        assert text[first] >= 0x80           # the sequence placed at 8192 - j is byte 0 of the batch: no low halo
        text = text[first:]
        return lay, text, symref.layout(0, "c", len(text))
    return lay, text, symref.layout(len(what), lay)


def same_results(r1, r2, what):
    for f in ARRAYS:
        assert np.array_equal(getattr(r1, f), getattr(r2, f)), (what, f)


def same_stream(s1, s2, what):
    assert np.array_equal(s1[0], s2[0]) and np.array_equal(s1[1], s2[1]) and s1[2] == s2[2], what


# ---------------------------------------------------------------- device-resident input (run in the child)
def _device_input(text, off, k):
    """The text in a device tensor of exactly k + total bytes, from byte k on (a pointer k bytes off a 4-byte
    boundary), and the offsets; torch's own work finished before the batch's stream reads them."""
    import torch
    buf = np.zeros(k + len(text), dtype=np.uint8)
    buf[k:] = text
    t_text = torch.from_numpy(buf).to("cuda")[k:]
    t_off = torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).to("cuda")
    torch.cuda.synchronize()
    assert t_text.data_ptr() % 4 == k and t_text.numel() == len(text)
    return t_text, t_off


def _set_device(b, text, off, k):
    t_text, t_off = _device_input(text, off, k)
    b.set_input_device(t_text.data_ptr(), t_off.data_ptr(), len(off) - 1, len(text), keep=(t_text, t_off), doc_off_host=off)


def _trim(text, off, m):
    """The batch without its last m bytes (the last document is that much shorter)."""
    if m == 0:
        return text, off
    off = off.copy()
    off[-1] -= m
    assert off[-1] > off[-2]
    return text[:len(text) - m], off


def _device_equals_host_and_reference(ctx, name, key, text, off, k, oracle_docs=None):
    import datok_amd
    tok, _, memo, _ = ctx.model(name)
    raw = text.tobytes()
    with datok_amd.Batch(len(text), len(off) - 1) as b, run_batch(tok, text, off) as host:
        _set_device(b, text, off, k)
        b.run(tok, 0)
        what = "%s: %s from a device pointer %d bytes off, %d bytes" % (name, key, k, len(text))
        stream, res = b.debug_stream(), b.result()
        symref.assert_stream_equal(stream, ctx.ref(name, key, text, off), text, off, what)
        same_stream(stream, host.debug_stream(), what)
        same_results(res, host.result(), what)
        docs = range(len(off) - 1) if oracle_docs is None else oracle_docs
        assert_batch_equals_oracle(memo, res, text, off, docs=docs)
        (data, o), (hdata, ho) = b.render(SIMPLE), host.render(SIMPLE)
        assert data == hdata and np.array_equal(o, ho), what
        for d in docs:
            exp, est = memo.transduce(raw[int(off[d]):int(off[d + 1])], SIMPLE)
            assert est == 0 and data[int(o[d]):int(o[d + 1])] == exp, (what, d)


def resident(ctx, name, k):
    """bench.py's path.  A caller's buffer is read with 4-byte loads only if its address and its size are multiples
    of 4 (k_symbolize<true, *> on a buffer without padding), else byte by byte (<false, *>): pointers 0..3 bytes off,
    sizes of every residue, exactly sized tensors; layouts (a) and (c) and the tails, codes and 16-bit entries.
    Stream, bitmap, flag, offsets and rendering equal the reference, and -- bit for bit -- the same text sent through
    set_input on another batch.  (Offsets and rendering against the oracle: every document of (a) and of the tails,
    every sixteenth of (c); all of them against the host-input batch.)"""
    for n in symref.TAILS:
        text, off = symref.tail(n)
        _device_equals_host_and_reference(ctx, name, "tail%d" % n, text, off, k)
    for lay in ("a", "c"):
        _, text, off = rows_batch(ctx, name, lay)
        for m in (0, 1 + k % 3):                             # sizes of every residue over the four pointers
            t, o = _trim(text, off, m)
            _device_equals_host_and_reference(ctx, name, "%s-%d" % (lay, m), t, o, k,
                                              None if lay == "a" else range(k, len(o) - 1, 16))
    assert {n % 4 for n in symref.TAILS} == {0, 1, 2, 3}


def alternate(ctx, name):
    """One batch, three inputs with identical offsets: the lane plan of the first host input may serve the third, but
    not across the device input between them, whose offsets live in another buffer."""
    import datok_amd
    tok, _, memo, _ = ctx.model(name)
    text, what = ctx.rows(name)
    per = 8
    off = symref.layout(per, "b")
    inputs = [text[i * per * symref.ROW:(i + 1) * per * symref.ROW] for i in (0, 3, 9)]
    with datok_amd.Batch(len(inputs[0]), len(off) - 1) as b:
        for turn in range(2):
            for i, (t, how) in enumerate(zip(inputs, ("host", "device", "host"))):
                if how == "host":
                    b.set_input(t, off)
                else:
                    _set_device(b, t, off, 1 + turn)
                b.run(tok, 0)
                what_ = "%s: input %d (%s), turn %d" % (name, i, how, turn)
                symref.assert_stream_equal(b.debug_stream(), ctx.ref(name, "alt%d" % i, t, off), t, off, what_)
                res = b.result()
                assert_batch_equals_oracle(memo, res, t, off)
                with run_batch(tok, t, off) as fresh:
                    same_results(res, fresh.result(), what_)
                    assert np.array_equal(res.ev_bits, fresh.result().ev_bits), what_


def rejected(ctx, previous):
    """dtk_batch_set_input_device checks the offsets before it touches the batch: after a rejected call the batch still
    holds its previous input, plan and host offsets, and a run reproduces the previous result."""
    import datok_amd
    import torch
    E_ARG, E_CAPACITY = datok_amd._lib.E_ARG, datok_amd._lib.E_CAPACITY
    name = SHIPPED[0]
    tok = ctx.model(name)[0]
    text, what = ctx.rows(name)
    text = text[:4 * symref.ROW]
    off = symref.layout(4, "b")
    n, total = len(off) - 1, len(text)
    other = np.ascontiguousarray(text[::-1])               # what a walk of the rejected buffers would see

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to("cuda")
    bad_first, bad_last, falling = off.copy(), off.copy(), off.copy()
    bad_first[0] = 5
    bad_last[-1] = total - 1
    falling[3], falling[4] = off[4], off[3]
    many = np.concatenate([off[:-1], np.full(8, off[-2]), off[-1:]])
    t_text = torch.from_numpy(other).to("cuda")
    cases = [("doc_off[0] != 0", dev(bad_first), n, total), ("doc_off[n] != total", dev(bad_last), n, total),
             ("a decreasing pair", dev(falling), n, total), ("n_docs > max_docs", dev(many), len(many) - 1, total),
             ("total > max_bytes", dev(off), n, total + 1)]
    torch.cuda.synchronize()
    with datok_amd.Batch(total, n) as b:
        if previous == "host":
            b.set_input(text, off)
        else:
            _set_device(b, text, off, 0)
        b.run(tok, 0)
        res0, stream0, render0 = b.result(), b.debug_stream(), b.render(SIMPLE)
        symref.assert_stream_equal(stream0, ctx.ref(name, "rejected", text, off), text, off, "before any rejected call")
        for what_, t_off, n_docs, total_bytes in cases:
            try:
                b.set_input_device(t_text.data_ptr(), t_off.data_ptr(), n_docs, total_bytes, keep=(t_text, t_off))
                raise AssertionError("accepted: " + what_)
            except datok_amd.DatokGpuError as e:
                assert e.code in (E_ARG, E_CAPACITY), (what_, e.code)
            assert (b.n_docs, b.total) == (n, total)
            b.run(tok, 0)
            same_results(b.result(), res0, what_)
            assert np.array_equal(b.result().ev_bits, res0.ev_bits), what_
            same_stream(b.debug_stream(), stream0, what_)
            data, o = b.render(SIMPLE)
            assert data == render0[0] and np.array_equal(o, render0[1]), what_


if __name__ == "__main__":
    import tempfile
    import torch
    torch.cuda.set_device(0)                  # torch's runtime first (see above)
    torch.cuda.synchronize()
    case, args = sys.argv[1], sys.argv[2:]
    with tempfile.TemporaryDirectory() as tmp:
        ctx = Ctx(tmp)
        if case == "resident":
            resident(ctx, args[0], int(args[1]))
        elif case == "alternate":
            alternate(ctx, args[0])
        elif case == "rejected":
            rejected(ctx, args[0])
        else:
            sys.exit("unknown case " + case)
        del ctx                               # (models and batches go before the runtimes do)
    print("DEVICE OK", case, *args)
