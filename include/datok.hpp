// datok.hpp -- C++ host mirror of Datok's public Go surface, on top of the
// C-ABI of libdatok_gpu.so (datok_gpu.h).  Header only.
//
// The reference is Go; no Go toolchain exists in the build image, so the host
// side above the C-ABI is C++ with the reference's names, argument meaning and
// error behaviour:
//
//   Go (reference)                                   here
//   ------------------------------------------------ ---------------------------------
//   Bits, TOKENS ... SIMPLE   token_writer.go:9-25   datok::Bits
//   TokenWriter{SentenceEnd,TextEnd,Flush,Token}     datok::TokenWriter (std::function)
//                             token_writer.go:27-33
//   NewTokenWriter(w, flags)  token_writer.go:36-175 datok::NewTokenWriter(std::ostream&, Bits)
//   Tokenizer interface       fomafile.go:29-33      datok::Tokenizer
//   LoadTokenizerFile(file)   fomafile.go:452-484    datok::LoadTokenizerFile -> nullptr + log on error
//   (*T).Transduce(r, w)      matrix.go:340-342      Tokenizer::Transduce(std::istream&, std::ostream&)
//   (*T).TransduceTokenWriter matrix.go:348-698      Tokenizer::TransduceTokenWriter(std::istream&, TokenWriter&)
//   (*T).Type()               matrix.go:102          Tokenizer::Type()
//   --                                               datok::ModelInfo(image, n, &info): the device layout a
//                                                    model file gets (dtk_model_info_mem; host only)
//
// The FSA walk itself runs on the GPU (dtk_batch_run); this header only drains
// the reader, calls the C-ABI and REPLAYS the returned events into the
// caller's four closures in the order the reference would have called them.
#pragma once

#include <cstdint>
#include <cstdio>
#include <functional>
#include <istream>
#include <iterator>
#include <memory>
#include <ostream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "datok_gpu.h"

namespace datok {

// token_writer.go:9-25
using Bits = uint8_t;
constexpr Bits TOKENS = 1, SENTENCES = 2, TOKEN_POS = 4, SENTENCE_POS = 8, NEWLINE_AFTER_EOT = 16,
               SIMPLE = TOKENS | SENTENCES;

using rune = char32_t;

// token_writer.go:27-33.  Token receives (offset, buf): buf is the rune window
// from its start to the end of the token, offset the number of leading runes
// that are not part of the token (skipped blanks), exactly as upstream.
struct TokenWriter {
  std::function<void(int)> SentenceEnd;
  std::function<void(int)> TextEnd;
  std::function<int()> Flush;
  std::function<void(int, const std::vector<rune> &)> Token;
};

namespace detail {

// Go unicode/utf8.DecodeRune
inline int decode_rune(const uint8_t *p, size_t n, rune *r) {
  *r = 0xFFFD;
  if (n == 0) return 0;
  uint32_t b0 = p[0];
  if (b0 < 0x80) { *r = b0; return 1; }
  if (b0 < 0xC2 || b0 > 0xF4) return 1;
  if (b0 < 0xE0) {
    if (n < 2 || (p[1] & 0xC0) != 0x80) return 1;
    *r = ((b0 & 0x1F) << 6) | (p[1] & 0x3F);
    return 2;
  }
  if (b0 < 0xF0) {
    uint32_t lo = b0 == 0xE0 ? 0xA0 : 0x80, hi = b0 == 0xED ? 0x9F : 0xBF;
    if (n < 3 || p[1] < lo || p[1] > hi || (p[2] & 0xC0) != 0x80) return 1;
    *r = ((b0 & 0x0F) << 12) | ((uint32_t)(p[1] & 0x3F) << 6) | (p[2] & 0x3F);
    return 3;
  }
  uint32_t lo = b0 == 0xF0 ? 0x90 : 0x80, hi = b0 == 0xF4 ? 0x8F : 0xBF;
  if (n < 4 || p[1] < lo || p[1] > hi || (p[2] & 0xC0) != 0x80 || (p[3] & 0xC0) != 0x80) return 1;
  *r = ((b0 & 0x07) << 18) | ((uint32_t)(p[1] & 0x3F) << 12) | ((uint32_t)(p[2] & 0x3F) << 6) |
       (p[3] & 0x3F);
  return 4;
}

// Go string(rune): invalid runes become U+FFFD
inline void append_rune(std::string &s, rune r) {
  if (r > 0x10FFFF || (r >= 0xD800 && r <= 0xDFFF)) r = 0xFFFD;
  if (r < 0x80) s.push_back((char)r);
  else if (r < 0x800) { s.push_back((char)(0xC0 | (r >> 6))); s.push_back((char)(0x80 | (r & 0x3F))); }
  else if (r < 0x10000) {
    s.push_back((char)(0xE0 | (r >> 12))); s.push_back((char)(0x80 | ((r >> 6) & 0x3F)));
    s.push_back((char)(0x80 | (r & 0x3F)));
  } else {
    s.push_back((char)(0xF0 | (r >> 18))); s.push_back((char)(0x80 | ((r >> 12) & 0x3F)));
    s.push_back((char)(0x80 | ((r >> 6) & 0x3F))); s.push_back((char)(0x80 | (r & 0x3F)));
  }
}

inline int count_runes(const uint8_t *p, size_t n) {
  int k = 0;
  size_t i = 0;
  rune r;
  while (i < n) { i += (size_t)decode_rune(p + i, n - i, &r); k++; }
  return k;
}

// Replays the events of document d of a host dtk_result_view (the bitmaps of ev_bits, the tail word, the
// token start offsets) into the closures.  Order at one cursor position: SEOT, TEOT, END, SEPS; the final
// SentenceEnd / TextEnd come last.  The int arguments follow the reference: the matrix passes buffc everywhere
// (matrix.go:575,597,600,684,691), the double array passes 0 except for the SentenceEnd fired by EOT
// (datok.go:1015,1023,1026,1119,1127).
inline void replay(bool is_matrix, const uint8_t *text, size_t n, const dtk_result_view &v, uint64_t doc_off_d,
                   uint32_t d, TokenWriter &w) {
  const uint64_t g0 = DTK_EVENT_BIT(doc_off_d, d);
  auto bit = [&](int kind, size_t p) {
    const uint64_t g = g0 + p;
    return (v.ev_bits[(uint64_t)kind * v.ev_words + (g >> 5)] >> (g & 31)) & 1u;
  };
  const uint32_t *tok_bstart = v.tok_bstart + v.tok_off[d];
  size_t B = 0;      // byte position of the window start (last rewind)
  size_t k = 0;      // tokens replayed so far (index into tok_bstart)
  std::vector<rune> buf;
  auto buffc = [&](size_t p) { return count_runes(text + B, p - B); };
  for (size_t p = 0; p <= n; p++) {
    if (bit(DTK_EVB_SEOT, p)) w.SentenceEnd(buffc(p));
    if (bit(DTK_EVB_TEOT, p)) {
      w.TextEnd(is_matrix ? buffc(p) : 0);
      if (is_matrix) B = p;  // matrix.go:601 rewinds, datok.go:1019-1030 does not
    }
    if (bit(DTK_EVB_END, p)) {
      const size_t start = tok_bstart[k++];
      buf.clear();
      int offset = 0;
      size_t i = B;
      while (i < p) {
        rune r;
        int wd = decode_rune(text + i, n - i, &r);
        if (i < start) offset++;
        buf.push_back(r);
        i += (size_t)wd;
      }
      w.Token(offset, buf);
      B = p;
    }
    if (bit(DTK_EVB_SEPS, p)) w.SentenceEnd(is_matrix ? buffc(p) : 0);
  }
  const uint32_t tail = v.doc_tail[d];
  const size_t pt = tail >> 2;
  if (tail & DTK_TAIL_S) w.SentenceEnd(is_matrix ? buffc(pt) : 0);
  if (tail & DTK_TAIL_E) w.TextEnd(is_matrix ? buffc(pt) : 0);
}

// The same from the event list of document d (DTK_R_EVENT_LIST: evl_off / evl_pos / evl_kind) instead of the bitmaps:
// the document's tokens and its entries are merged by cursor position -- O(tokens + entries), where replay() tests
// four bits at every byte.  A token's cursor is tok_bend[k] and its first byte tok_bstart[k]; where only the blocked
// byte offsets were delivered (DTK_R_TOK_BYTE_BLK) both come from dtk_blk_end / dtk_blk_start.  Order and int
// arguments as above.
// A slice of a stream (dtk_stream_slice) is replayed the same way into the stream's one writer: the window start
// begins at the slice's `first` instead of 0, and the tail word counts on the last slice only.
inline void replay_list(bool is_matrix, const uint8_t *text, size_t n, const dtk_result_view &v, uint32_t d,
                        TokenWriter &w, size_t first = 0, bool with_tail = true) {
  const uint64_t t0 = v.tok_off[d], t1 = v.tok_off[d + 1];
  const bool blocked = !v.tok_bend && v.tok_bblk;
  auto tok_end = [&](uint64_t i) { return blocked ? (size_t)dtk_blk_end(v.tok_bblk, v.tok_bblk_head, i) : (size_t)v.tok_bend[i]; };
  auto tok_start = [&](uint64_t i) { return blocked ? (size_t)dtk_blk_start(v.tok_bblk, v.tok_bblk_head, i) : (size_t)v.tok_bstart[i]; };
  uint64_t k = t0;                               // next token
  uint32_t j = v.evl_off[d];                     // next entry
  const uint32_t j1 = v.evl_off[d + 1];
  size_t B = first;                              // byte position of the window start (last rewind)
  std::vector<rune> buf;
  auto buffc = [&](size_t p) { return count_runes(text + B, p - B); };
  while (k < t1 || j < j1) {
    const size_t none = n + 1;
    const size_t pt = k < t1 ? tok_end(k) : none, pe = j < j1 ? (size_t)v.evl_pos[j] : none;
    const size_t p = pt < pe ? pt : pe;
    const uint32_t e = pe == p ? v.evl_kind[j++] : 0u;
    if (e & DTK_EVL_SEOT) w.SentenceEnd(buffc(p));
    if (e & DTK_EVL_TEOT) {
      w.TextEnd(is_matrix ? buffc(p) : 0);
      if (is_matrix) B = p;  // matrix.go:601 rewinds, datok.go:1019-1030 does not
    }
    if (pt == p) {
      const size_t start = tok_start(k++);
      buf.clear();
      int offset = 0;
      size_t i = B;
      while (i < p) {
        rune r;
        int wd = decode_rune(text + i, n - i, &r);
        if (i < start) offset++;
        buf.push_back(r);
        i += (size_t)wd;
      }
      w.Token(offset, buf);
      B = p;
    }
    if (e & DTK_EVL_SEPS) w.SentenceEnd(is_matrix ? buffc(p) : 0);
  }
  if (!with_tail) return;
  const uint32_t tail = v.doc_tail[d];
  const size_t pt = tail >> 2;
  if (tail & DTK_TAIL_S) w.SentenceEnd(is_matrix ? buffc(pt) : 0);
  if (tail & DTK_TAIL_E) w.TextEnd(is_matrix ? buffc(pt) : 0);
}

// The same for a document walked by the exact pass (dtk_result_view.calls): the calls are listed in
// the reference's order with their arguments.
inline void replay_calls(const uint8_t *text, size_t n, const dtk_call *calls, size_t n_calls, TokenWriter &w) {
  std::vector<rune> buf;
  for (size_t k = 0; k < n_calls; k++) {
    const dtk_call &c = calls[k];
    if (c.kind == 0) {
      buf.clear();
      int offset = 0;
      size_t i = (size_t)c.a;
      while (i < c.c && i < n) {
        rune r;
        int wd = decode_rune(text + i, n - i, &r);
        if (i < c.b) offset++;
        buf.push_back(r);
        i += (size_t)wd;
      }
      if (c.b > c.c) offset += count_runes(text + c.c, (c.b < n ? c.b : n) - c.c);  // DTK_ST_BAD_OFFSET: offset > len(buf)
      w.Token(offset, buf);
    } else if (c.kind == 1) {
      w.SentenceEnd(c.a);
    } else {
      w.TextEnd(c.a);
    }
  }
}

// document 0 of a one-stream batch (host view): its event bitmaps, or the call list if the exact pass walked it
inline void replay_view(bool is_matrix, const uint8_t *text, size_t n, const dtk_result_view &v, TokenWriter &w) {
  if (v.n_exact && v.exact_doc[0] == 0)
    replay_calls(text, n, v.calls + v.exact_off[0], (size_t)(v.exact_off[1] - v.exact_off[0]), w);
  else
    replay(is_matrix, text, n, v, 0, 0, w);
}

}  // namespace detail

// token_writer.go:36-175
inline std::unique_ptr<TokenWriter> NewTokenWriter(std::ostream &w, Bits flags) {
  struct State {
    int posC = 0;
    std::vector<int> pos, sent;
    bool sentB = true, init = true;
    std::string out;  // bufio.Writer
  };
  auto st = std::make_shared<State>();
  auto tw = std::make_unique<TokenWriter>();
  std::ostream *os = &w;
  auto flush = [st, os]() {
    os->write(st->out.data(), (std::streamsize)st->out.size());
    st->out.clear();
    os->flush();
    return os->good() ? 0 : -1;
  };
  auto surface = [st](int offset, const std::vector<rune> &buf) {
    for (size_t i = (size_t)offset; i < buf.size(); i++) detail::append_rune(st->out, buf[i]);
    st->out.push_back('\n');
  };

  if (flags & (TOKEN_POS | SENTENCE_POS)) {  // :49-88
    tw->Token = [st, flags, surface](int offset, const std::vector<rune> &buf) {
      if (st->posC == 0 && (flags & NEWLINE_AFTER_EOT) && !buf.empty() && buf[0] == U'\n' && !st->init)
        st->posC--;
      st->init = false;
      st->posC += offset;
      st->pos.push_back(st->posC);
      if (st->sentB) { st->sentB = false; st->sent.push_back(st->posC); }
      st->posC += (int)buf.size() - offset;
      st->pos.push_back(st->posC);
      if (flags & TOKENS) surface(offset, buf);
    };
  } else if (flags & TOKENS) {  // :91-95
    tw->Token = [surface](int offset, const std::vector<rune> &buf) { surface(offset, buf); };
  } else {
    tw->Token = [](int, const std::vector<rune> &) {};
  }

  if (flags & SENTENCE_POS) {  // :103-115 (Go panics on an empty pos; we skip the append)
    tw->SentenceEnd = [st, flags](int) {
      if (!st->pos.empty()) st->sent.push_back(st->pos.back());
      st->sentB = true;
      if (flags & SENTENCES) st->out.push_back('\n');
    };
  } else if (flags & SENTENCES) {  // :118-122
    tw->SentenceEnd = [st, flush](int) { st->out.push_back('\n'); flush(); };
  } else {
    tw->SentenceEnd = [](int) {};
  }

  if (flags & (TOKEN_POS | SENTENCE_POS)) {  // :130-159
    tw->TextEnd = [st, flags, flush](int) {
      auto ints = [st](const std::vector<int> &v) {
        for (size_t i = 0; i < v.size(); i++) {
          if (i) st->out.push_back(' ');
          st->out += std::to_string(v[i]);
        }
        st->out.push_back('\n');
      };
      if ((flags & TOKEN_POS) && !st->pos.empty()) ints(st->pos);
      if (flags & SENTENCE_POS) {
        if (!st->sent.empty()) ints(st->sent);
        st->sent.clear();
        st->sentB = true;
      }
      flush();
      st->posC = 0;
      st->pos.clear();
    };
  } else {  // :162-166
    tw->TextEnd = [st, flush](int) { st->out.push_back('\n'); flush(); };
  }
  tw->Flush = flush;  // :170-172
  return tw;
}

// fomafile.go:29-33
class Tokenizer {
 public:
  virtual ~Tokenizer() = default;
  virtual bool Transduce(std::istream &r, std::ostream &w) = 0;
  virtual bool TransduceTokenWriter(std::istream &r, TokenWriter &w) = 0;
  virtual std::string Type() const = 0;
};

// MatrixTokenizer / DaTokenizer behind one class: the encoding is a property of
// the loaded file (matrix.go:16-26, datok.go:63-76).
class GpuTokenizer final : public Tokenizer {
 public:
  explicit GpuTokenizer(dtk_model *m) : m_(m) {}
  ~GpuTokenizer() override { dtk_model_free(m_); }
  GpuTokenizer(const GpuTokenizer &) = delete;
  GpuTokenizer &operator=(const GpuTokenizer &) = delete;

  std::string Type() const override { return dtk_model_type(m_); }
  const dtk_model *model() const { return m_; }

  // matrix.go:340-342 / datok.go:769-771: TransduceTokenWriter(r, NewTokenWriter(w, SIMPLE)).
  // The stock writer's bytes are rendered on the device (dtk_transduce); a custom writer goes
  // through TransduceTokenWriter below.
  bool Transduce(std::istream &r, std::ostream &w) override { return TransduceBits(r, w, SIMPLE); }

  // TransduceTokenWriter(r, NewTokenWriter(w, bits)) for any Bits
  bool TransduceBits(std::istream &r, std::ostream &w, Bits bits) {
    std::string text((std::istreambuf_iterator<char>(r)), std::istreambuf_iterator<char>());
    char *out = nullptr;
    size_t n = 0;
    last_status_ = 0;
    if (dtk_transduce(m_, (const uint8_t *)text.data(), text.size(), (uint32_t)bits, &out, &n, &last_status_) != DTK_OK)
      return false;
    w.write(out, (std::streamsize)n);
    w.flush();
    dtk_free(out);
    return true;
  }

  // matrix.go:348-698 / datok.go:781-1135: one stream = one document.
  bool TransduceTokenWriter(std::istream &r, TokenWriter &w) override {
    std::string text((std::istreambuf_iterator<char>(r)), std::istreambuf_iterator<char>());
    last_status_ = 0;
    const bool ok = TransduceBytes((const uint8_t *)text.data(), text.size(), w);
    w.Flush();  // `defer w.Flush()`, matrix.go:374
    return ok;
  }

  bool TransduceBytes(const uint8_t *text, size_t n, TokenWriter &w) {
    dtk_result_view v;  // on the calling thread's cached batch
    const bool ok = dtk_transduce_result(m_, text, n, 0, &v) == DTK_OK;
    if (ok) {
      last_status_ = v.status[0];
      detail::replay_view(Type() == "MATOK", text, n, v, w);
      // the reference cannot finish such a document whatever the writer does (matrix.go:365,406 index panic,
      // a walk that left the table): false
      if (last_status_ & (DTK_ST_WINDOW_OVERFLOW | DTK_ST_BAD_MODEL | DTK_ST_STEP_LIMIT | DTK_ST_INTERNAL | DTK_ST_IRREGULAR))
        return false;
    }
    return ok;
  }
  // The same for a reader of any length, as the reference reads it through a bufio.Reader (matrix.go:373): the stream
  // is read and walked in slices of slice_bytes (dtk_stream_run: host memory stays at depth * (slice_bytes + 8192)
  // bytes) and replayed slice by slice into the one writer.  false also for a stream a slice of which needs the exact
  // pass (DTK_E_IRREGULAR: crafted models only).
  bool TransduceStream(std::istream &r, TokenWriter &w, uint64_t slice_bytes = 16u << 20, uint32_t depth = 3) {
    last_status_ = 0;
    dtk_stream *s = nullptr;
    if (dtk_stream_create(slice_bytes, depth, &s) != DTK_OK) return false;
    const int rc = RunStream(s, r, w);
    dtk_stream_free(s);
    w.Flush();  // `defer w.Flush()`, matrix.go:374
    return rc == DTK_OK &&
           !(last_status_ & (DTK_ST_WINDOW_OVERFLOW | DTK_ST_BAD_MODEL | DTK_ST_STEP_LIMIT | DTK_ST_INTERNAL | DTK_ST_IRREGULAR));
  }
  // TransduceTokenWriter(r, NewTokenWriter(w, bits)) for a reader of any length: every slice's bytes are rendered on
  // the device and written to w as they come home -- no closure is called.  Without a position flag the writer keeps
  // no state (dtk_stream_set_render); with TOKEN_POS or SENTENCE_POS its state is carried on the device
  // (dtk_stream_set_position_render) and dtk_stream_emit holds the position line of the text that is open.
  bool TransduceStream(std::istream &r, std::ostream &w, Bits bits, uint64_t slice_bytes = 16u << 20, uint32_t depth = 3) {
    last_status_ = 0;
    dtk_stream *s = nullptr;
    if (dtk_stream_create(slice_bytes, depth, &s) != DTK_OK) return false;
    const bool positions = (bits & (TOKEN_POS | SENTENCE_POS)) != 0;
    int rc = positions ? dtk_stream_set_position_render(s, 1, (uint32_t)bits) : dtk_stream_set_render(s, 1, (uint32_t)bits);
    // (the blocked token bytes: nobody reads them here)
    if (rc == DTK_OK) rc = dtk_stream_set_result_fields(s, DTK_R_TOK_BYTE_BLK);
    if (rc == DTK_OK) {
      struct Ctx { std::istream *r; std::ostream *w; dtk_stream *s; bool positions; } c{&r, &w, s, positions};
      auto rd = [](void *u, uint8_t *buf, size_t cap) -> size_t {
        Ctx *c = static_cast<Ctx *>(u);
        c->r->read(reinterpret_cast<char *>(buf), (std::streamsize)cap);
        return (size_t)c->r->gcount();
      };
      auto on_slice = [](void *u, const dtk_stream_slice *sl) -> int {
        Ctx *c = static_cast<Ctx *>(u);
        const dtk_write_fn wr = [](void *o, const uint8_t *p, size_t n) -> int {
          static_cast<std::ostream *>(o)->write(reinterpret_cast<const char *>(p), (std::streamsize)n);
          return DTK_OK;
        };
        return c->positions ? dtk_stream_emit(c->s, wr, c->w) : wr(c->w, sl->out, (size_t)sl->out_len);
      };
      rc = dtk_stream_run(s, m_, rd, &c, (uint32_t)bits & DTK_NEWLINE_AFTER_EOT, on_slice, &c, &last_status_);
    }
    dtk_stream_free(s);
    w.flush();
    if (!positions) last_status_ &= ~(uint32_t)DTK_ST_EMPTY_TEXT;  // (an empty text only breaks the position modes)
    return rc == DTK_OK &&
           !(last_status_ & (DTK_ST_WINDOW_OVERFLOW | DTK_ST_BAD_MODEL | DTK_ST_STEP_LIMIT | DTK_ST_INTERNAL | DTK_ST_IRREGULAR));
  }
  // The rune offsets and sentence list of a reader of any length as data, for a caller that reads offsets and not text
  // (what a NewTokenWriter with TOKEN_POS | SENTENCE_POS collects, newline_after_eot as its NEWLINE_AFTER_EOT):
  // cb(const dtk_stream_slice &, const dtk_stream_offs &) gets every slice's arrays in order (dtk_stream_set_offsets;
  // form: DTK_SO_PLAIN or DTK_SO_BLOCKED, decode with dtk_blk64_start / dtk_blk64_end where tok_rstart is null); they
  // are valid inside the call.  A non-zero return of cb ends the run.  No closure is called and no text is rendered.
  template <class Callback>
  bool TransduceStreamOffsets(std::istream &r, Callback &&cb, bool newline_after_eot = false, uint32_t form = DTK_SO_PLAIN,
                              uint64_t slice_bytes = 16u << 20, uint32_t depth = 3) {
    last_status_ = 0;
    dtk_stream *s = nullptr;
    if (dtk_stream_create(slice_bytes, depth, &s) != DTK_OK) return false;
    int rc = dtk_stream_set_offsets(s, 1, form);
    if (rc == DTK_OK) rc = dtk_stream_set_result_fields(s, DTK_R_TOK_BYTE_BLK);
    if (rc == DTK_OK) {
      struct Ctx { std::istream *r; dtk_stream *s; typename std::remove_reference<Callback>::type *cb; } c{&r, s, &cb};
      auto rd = [](void *u, uint8_t *buf, size_t cap) -> size_t {
        Ctx *c = static_cast<Ctx *>(u);
        c->r->read(reinterpret_cast<char *>(buf), (std::streamsize)cap);
        return (size_t)c->r->gcount();
      };
      auto on_slice = [](void *u, const dtk_stream_slice *sl) -> int {
        Ctx *c = static_cast<Ctx *>(u);
        dtk_stream_offs o;
        const int rc = dtk_stream_offsets(c->s, &o);
        return rc != DTK_OK ? rc : (int)(*c->cb)(*sl, o);
      };
      rc = dtk_stream_run(s, m_, rd, &c, newline_after_eot ? (uint32_t)DTK_NEWLINE_AFTER_EOT : 0u, on_slice, &c, &last_status_);
    }
    dtk_stream_free(s);
    return rc == DTK_OK &&
           !(last_status_ & (DTK_ST_WINDOW_OVERFLOW | DTK_ST_BAD_MODEL | DTK_ST_STEP_LIMIT | DTK_ST_INTERNAL | DTK_ST_IRREGULAR));
  }
  // The sentences of a reader of any length as rows, for a caller that wants sentence spans and no token offsets:
  // cb(const dtk_stream_slice &, const dtk_stream_sens &) gets the rows every slice's calls close, in order
  // (dtk_stream_set_sentences: the slices' rows one behind the other are the stream's table; the row open at a cut is
  // carried on the device); they are valid inside the call.  newline_after_eot moves the rune spans as it moves the
  // writer's offsets.  A non-zero return of cb ends the run.  No closure is called, no text is rendered and no token
  // offsets come home.
  template <class Callback>
  bool TransduceStreamSentences(std::istream &r, Callback &&cb, bool newline_after_eot = false,
                                uint64_t slice_bytes = 16u << 20, uint32_t depth = 3) {
    last_status_ = 0;
    dtk_stream *s = nullptr;
    if (dtk_stream_create(slice_bytes, depth, &s) != DTK_OK) return false;
    int rc = dtk_stream_set_sentences(s, 1);
    if (rc == DTK_OK) rc = dtk_stream_set_result_fields(s, DTK_R_TOK_BYTE_BLK);
    if (rc == DTK_OK) {
      struct Ctx { std::istream *r; dtk_stream *s; typename std::remove_reference<Callback>::type *cb; } c{&r, s, &cb};
      auto rd = [](void *u, uint8_t *buf, size_t cap) -> size_t {
        Ctx *c = static_cast<Ctx *>(u);
        c->r->read(reinterpret_cast<char *>(buf), (std::streamsize)cap);
        return (size_t)c->r->gcount();
      };
      auto on_slice = [](void *u, const dtk_stream_slice *sl) -> int {
        Ctx *c = static_cast<Ctx *>(u);
        dtk_stream_sens o;
        const int rc = dtk_stream_sentences(c->s, &o);
        return rc != DTK_OK ? rc : (int)(*c->cb)(*sl, o);
      };
      rc = dtk_stream_run(s, m_, rd, &c, newline_after_eot ? (uint32_t)DTK_NEWLINE_AFTER_EOT : 0u, on_slice, &c, &last_status_);
    }
    dtk_stream_free(s);
    last_status_ &= ~(uint32_t)DTK_ST_EMPTY_TEXT;  // (an empty text only breaks the position modes: it makes no row)
    return rc == DTK_OK &&
           !(last_status_ & (DTK_ST_WINDOW_OVERFLOW | DTK_ST_BAD_MODEL | DTK_ST_STEP_LIMIT | DTK_ST_INTERNAL | DTK_ST_IRREGULAR));
  }
  // ... on a dtk_stream the caller keeps (and has configured); returns dtk_stream_run's code
  int RunStream(dtk_stream *s, std::istream &r, TokenWriter &w) {
    struct Ctx { std::istream *r; TokenWriter *w; bool is_matrix; } c{&r, &w, Type() == "MATOK"};
    auto rd = [](void *u, uint8_t *buf, size_t cap) -> size_t {
      Ctx *c = static_cast<Ctx *>(u);
      c->r->read(reinterpret_cast<char *>(buf), (std::streamsize)cap);
      return (size_t)c->r->gcount();
    };
    auto on_slice = [](void *u, const dtk_stream_slice *sl) -> int {
      Ctx *c = static_cast<Ctx *>(u);
      detail::replay_list(c->is_matrix, sl->text, sl->len, sl->view, 0, *c->w, sl->first, sl->last != 0);
      return DTK_OK;
    };
    return dtk_stream_run(s, m_, rd, &c, 0, on_slice, &c, &last_status_);
  }
  uint32_t last_status() const { return last_status_; }

 private:
  dtk_model *m_;
  uint32_t last_status_ = 0;
};

// fomafile.go:452-484: nil + log line on any failure.
inline std::unique_ptr<Tokenizer> LoadTokenizerFile(const std::string &file) {
  dtk_model *m = nullptr;
  const int rc = dtk_model_load(file.c_str(), &m);
  if (rc != DTK_OK) {
    std::fprintf(stderr, "datok: %s: %s\n", file.c_str(), dtk_strerror(rc));
    return nullptr;
  }
  return std::make_unique<GpuTokenizer>(m);
}

// Which table and loop a model image (.matok / .datok / Foma net, gzip'd) gets on the device, decided as the loader
// decides it and without a device (dtk_model_info_mem): false + log line for an image the loader would reject.
// out->lean_walk says which loop (1: the lean one), out->stream_codes which stream format (0: 16-bit entries).
inline bool ModelInfo(const void *gz_bytes, size_t n, dtk_model_info *out) {
  const int rc = dtk_model_info_mem(gz_bytes, n, out);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: model image: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// ---- a batch's sentences as rows (dtk_sentence_view, datok_gpu.h): a sentence is a maximal non-empty run of Token
// calls with no SentenceEnd / TextEnd between them.
// The last run's table in page-locked host memory (device: device pointers), valid until the batch's next run; false +
// log line on failure (before a run, or after a run with DTK_NO_BYTE_OFFSETS).
inline bool Sentences(dtk_batch *b, dtk_sentence_view *out, bool device = false) {
  const int rc = device ? dtk_batch_sentences_device(b, out) : dtk_batch_sentences_host(b, out);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: sentences: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// One sentence of a document: its tokens [tok_first, tok_end) (document-relative, as text_tok_end counts), its bytes
// [bstart, bend) of the document and its runes [rstart, rend) of the text (0 when the run had DTK_NO_RUNE_OFFSETS).
struct SentenceRow {
  uint32_t tok_first, tok_end, bstart, bend;
  int32_t rstart, rend;
};
// The rows of document d of a host view.
inline std::vector<SentenceRow> sentence_rows(const dtk_sentence_view &v, uint32_t d) {
  std::vector<SentenceRow> rows;
  rows.reserve((size_t)(v.sen_off[d + 1] - v.sen_off[d]));
  uint32_t first = 0;
  for (uint64_t i = v.sen_off[d]; i < v.sen_off[d + 1]; i++) {
    rows.push_back(SentenceRow{first, v.sen_tok_end[i], v.sen_bstart[i], v.sen_bend[i], v.sen_rstart ? v.sen_rstart[i] : 0,
                               v.sen_rend ? v.sen_rend[i] : 0});
    first = v.sen_tok_end[i];
  }
  return rows;
}

// ---- every token looked up in a vocabulary on the device (dtk_vocab, dtk_tally, datok_gpu.h): type ids and a
// frequency list.  A token's id is the index of the word equal to its surface as the writer prints it (invalid bytes
// as U+FFFD), the lowest one of equal words, or DTK_ID_UNKNOWN.
class Vocab {
 public:
  // ok() is false, with a log line, when the table could not be made (no device, more than 2^31 - 2 words, 2^32 bytes).
  explicit Vocab(const std::vector<std::string> &words) {
    std::string bytes;
    std::vector<uint64_t> off(1, 0);
    for (const std::string &w : words) { bytes += w; off.push_back(bytes.size()); }
    const int rc = dtk_vocab_create(reinterpret_cast<const uint8_t *>(bytes.data()), off.data(), (uint32_t)words.size(), &v_);
    if (rc != DTK_OK) std::fprintf(stderr, "datok: vocabulary: %s\n", dtk_strerror(rc));
  }
  ~Vocab() { dtk_vocab_free(v_); }
  Vocab(const Vocab &) = delete;
  Vocab &operator=(const Vocab &) = delete;
  bool ok() const { return v_ != nullptr; }
  uint32_t size() const { return dtk_vocab_size(v_); }
  const dtk_vocab *get() const { return v_; }

 private:
  dtk_vocab *v_ = nullptr;
};

// The counters of a frequency list beside a Vocab: attach with dtk_batch_set_vocab / dtk_pipeline_set_vocab /
// dtk_stream_set_vocab; every run adds its tokens once.
class Tally {
 public:
  explicit Tally(const Vocab &v) : n_(v.size()) {
    const int rc = dtk_tally_create(v.get(), &t_);
    if (rc != DTK_OK) std::fprintf(stderr, "datok: tally: %s\n", dtk_strerror(rc));
  }
  ~Tally() { dtk_tally_free(t_); }
  Tally(const Tally &) = delete;
  Tally &operator=(const Tally &) = delete;
  bool ok() const { return t_ != nullptr; }
  dtk_tally *get() const { return t_; }
  // size() + 1 counts, the last one the unknown tokens'; empty on failure
  std::vector<uint64_t> read() const {
    std::vector<uint64_t> counts((size_t)n_ + 1);
    if (!t_ || dtk_tally_read(t_, counts.data()) != DTK_OK) counts.clear();
    return counts;
  }
  bool reset() { return t_ && dtk_tally_reset(t_) == DTK_OK; }

 private:
  dtk_tally *t_ = nullptr;
  uint32_t n_ = 0;
};

// The last run's ids in page-locked host memory (device: device pointers), valid until the batch's next run; false + log
// line on failure (before a run, without a vocabulary, or after a run with DTK_NO_BYTE_OFFSETS).
inline bool token_ids(dtk_batch *b, dtk_token_id_view *out, bool device = false) {
  const int rc = device ? dtk_batch_token_ids_device(b, out) : dtk_batch_token_ids_host(b, out);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: token ids: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// ---- every token split into WordPiece ids over a Vocab on the device (dtk_batch_set_wordpiece, datok_gpu.h): greedy
// longest-match-first, continuation pieces looked up behind `prefix`; a token that cannot be split, or has more than
// max_runes runes, is the single piece unk_id.
struct WordPiece {
  std::string prefix = "##";   // 0..16 bytes
  int32_t unk_id = 0;          // 0 <= unk_id < the vocabulary's size
  uint32_t max_runes = 0;      // 0: 100, BERT's max_input_chars_per_word
  bool pieces_home = true;     // the pieces come home with the batch's other result copies
};

// Attaches the split to a batch (v == nullptr: off); false + log line for options outside their ranges.
inline bool set_wordpiece(dtk_batch *b, const Vocab *v, const WordPiece &o = WordPiece()) {
  const int rc = dtk_batch_set_wordpiece(b, v ? v->get() : nullptr, reinterpret_cast<const uint8_t *>(o.prefix.data()),
                                         (uint32_t)o.prefix.size(), o.unk_id, o.max_runes, o.pieces_home ? 1 : 0);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: wordpiece: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// The last run's pieces in page-locked host memory (device: device pointers), valid until the batch's next run: token
// i's are piece_id[piece_off[i] .. piece_off[i + 1]).  false + log line on failure (before a run, without a split, or
// after a run with DTK_NO_BYTE_OFFSETS).
inline bool pieces(dtk_batch *b, dtk_piece_view *out, bool device = false) {
  const int rc = device ? dtk_batch_pieces_device(b, out) : dtk_batch_pieces_host(b, out);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: pieces: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// ---- token keys folded on the device (dtk_fold, datok_gpu.h): a finite map from a code point to 0..DTK_FOLD_MAX code
// points, applied rune by rune where the lookup (Vocab) and the split (WordPiece) read a token's key -- lower-casing and
// accent stripping for uncased vocabularies -- with every offset still counted in source bytes.  The vocabulary is not
// folded: it must be in folded form already.  The map is data; code points it does not list fold to themselves.
class Fold {
 public:
  // ok() is false, with a log line, when the fold could not be made (no device, a surrogate or a duplicate source, more
  // than DTK_FOLD_MAX targets, a target that is no scalar value).
  explicit Fold(const std::vector<std::pair<uint32_t, std::u32string>> &mapping) {
    std::vector<uint32_t> from, to_off(1, 0), to;
    for (const auto &m : mapping) {
      from.push_back(m.first);
      for (char32_t c : m.second) to.push_back((uint32_t)c);
      to_off.push_back((uint32_t)to.size());
    }
    from.push_back(0); to.push_back(0);  // (never read: the arrays are not null for an empty mapping)
    const int rc = dtk_fold_create(from.data(), to_off.data(), to.data(), (uint32_t)mapping.size(), &f_);
    if (rc != DTK_OK) std::fprintf(stderr, "datok: fold: %s\n", dtk_strerror(rc));
  }
  ~Fold() { dtk_fold_free(f_); }
  Fold(const Fold &) = delete;
  Fold &operator=(const Fold &) = delete;
  bool ok() const { return f_ != nullptr; }
  const dtk_fold *get() const { return f_; }

 private:
  dtk_fold *f_ = nullptr;
};

// Attaches the fold to a batch's ids and split (f == nullptr: off); the finished run's ids, pieces and rows are computed
// anew under it when they are next asked for.  false + log line for a fold of another device.
inline bool set_fold(dtk_batch *b, const Fold *f) {
  const int rc = dtk_batch_set_fold(b, f ? f->get() : nullptr);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: fold: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// ---- sentences or documents as fixed-length model input rows on the device (dtk_batch_set_encode, datok_gpu.h): behind
// the WordPiece split, cls_id / the unit's pieces / sep_id / pad_id up to max_len; a unit with more pieces than a row's
// body is cut into windows that share `stride` pieces.
struct EncodeSpec {
  uint32_t max_len = 128;                 // the row width, counted with the special positions (at most 65 535)
  int32_t cls_id = -1, sep_id = -1;       // -1: the position does not exist
  int32_t pad_id = 0;
  uint32_t unit = DTK_ENC_SENTENCE;       // or DTK_ENC_DOCUMENT
  uint32_t stride = 0;                    // 0 <= stride < max_len - n_special
  bool first_window = false;              // keep only window 0 of every unit: plain truncation
  bool word_ids = false;                  // also deliver word_id
  bool rows_home = true;                  // the rows come home with the batch's other result copies
};

// Attaches the encoding to a batch (spec == nullptr: off); false + log line for a spec outside its ranges.
inline bool set_encode(dtk_batch *b, const EncodeSpec *spec) {
  dtk_encode_spec s{};
  if (spec)
    s = dtk_encode_spec{spec->max_len, spec->cls_id, spec->sep_id, spec->pad_id, spec->unit, spec->stride,
                        (spec->first_window ? (uint32_t)DTK_ENC_FIRST_WINDOW : 0u) | (spec->word_ids ? (uint32_t)DTK_ENC_WORD_IDS : 0u)};
  const int rc = dtk_batch_set_encode(b, spec ? &s : nullptr, spec && spec->rows_home ? 1 : 0);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: encode: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

// The last run's rows in page-locked host memory (device: device pointers), valid until the batch's next run: row
// unit_row_off[u] + k is window k of unit u, input_ids[r * max_len + p] its position p.  false + log line on failure
// (before a run, without an encoding, without a split, or after a run with DTK_NO_BYTE_OFFSETS).
inline bool encoded(dtk_batch *b, dtk_encode_view *out, bool device = false) {
  const int rc = device ? dtk_batch_encoded_device(b, out) : dtk_batch_encoded_host(b, out);
  if (rc != DTK_OK) std::fprintf(stderr, "datok: encoded: %s\n", dtk_strerror(rc));
  return rc == DTK_OK;
}

}  // namespace datok
