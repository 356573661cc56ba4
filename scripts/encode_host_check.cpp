// encode_host_check.cpp -- the encoding rule (datok_amd/csrc/dtk_encode.cpp, dtk_encode_core.h) in a program of its
// own, for a run under the host sanitizers.  It makes no HIP call and needs no device:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o encode_host_check \
//         scripts/encode_host_check.cpp datok_amd/csrc/dtk_encode.cpp && ./encode_host_check
//
// The grid of tests/test_encode_host.py -- units of 0..3 * body pieces, every stride, max_len in {1 + n_special, 4, 5, 8},
// the four choices of specials, with and without FIRST_WINDOW and word_id, tokens of 1, 0, 2 and 5 pieces -- goes through
// dtk_encode_rows_mem and is compared with a plain restatement of the definition.  Every output array is allocated at
// exactly the needed size, so a row written behind it is seen; so is a call with one row too few (DTK_E_CAPACITY).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/datok_gpu.h"

namespace {
long checked = 0;

struct Batch {
  std::vector<uint64_t> piece_off{0}, ends, tok_off{0};
  std::vector<int32_t> piece_id;
};

// units of ns[i] pieces, three to a document
Batch make(const std::vector<unsigned> &ns) {
  static const unsigned kTokens[4] = {1, 0, 2, 5};
  Batch b;
  for (size_t i = 0; i < ns.size(); i++) {
    if (i && i % 3 == 0) b.tok_off.push_back(b.piece_off.size() - 1);
    unsigned left = ns[i], k = 0;
    if (!left && i % 2) b.piece_off.push_back(b.piece_off.back());
    while (left) {
      const unsigned c = kTokens[k++ % 4] < left ? kTokens[(k - 1) % 4] : left;
      b.piece_off.push_back(b.piece_off.back() + c);
      left -= c;
    }
    b.ends.push_back(b.piece_off.size() - 1);
  }
  b.tok_off.push_back(b.piece_off.size() - 1);
  for (uint64_t q = 0; q < b.piece_off.back(); q++) b.piece_id.push_back(100 + (int32_t)q);
  return b;
}

struct Rows {
  std::vector<uint64_t> off, piece0;
  std::vector<int32_t> ids, words;
  std::vector<uint32_t> len;
};

// The definition, restated.
Rows expected(const dtk_encode_spec &s, const Batch &b) {
  const unsigned has_cls = s.cls_id >= 0, has_sep = s.sep_id >= 0, body = s.max_len - has_cls - has_sep, step = body - s.stride;
  Rows r;
  size_t doc = 0;
  for (size_t u = 0; u < b.ends.size(); u++) {
    const uint64_t t0 = u ? b.ends[u - 1] : 0, t1 = b.ends[u], p0 = b.piece_off[t0], n = b.piece_off[t1] - p0;
    while (doc + 1 < b.tok_off.size() - 1 && b.tok_off[doc + 1] <= t0 && t0 < t1) doc++;
    r.off.push_back(r.len.size());
    const uint64_t w = n <= body || (s.flags & DTK_ENC_FIRST_WINDOW) ? 1 : 1 + (n - body + step - 1) / step;
    for (uint64_t k = 0; k < w; k++) {
      const uint64_t first = k * step, end = first + body < n ? first + body : n;
      std::vector<int32_t> row, word;
      if (has_cls) { row.push_back(s.cls_id); word.push_back(-1); }
      for (uint64_t q = p0 + first; q < p0 + end; q++) {
        row.push_back(b.piece_id[q]);
        uint64_t t = t0;
        while (!(b.piece_off[t] <= q && q < b.piece_off[t + 1])) t++;
        word.push_back((int32_t)(t - b.tok_off[doc]));
      }
      if (has_sep) { row.push_back(s.sep_id); word.push_back(-1); }
      r.len.push_back((uint32_t)row.size());
      r.piece0.push_back(p0 + first);
      row.resize(s.max_len, s.pad_id);
      word.resize(s.max_len, -1);
      r.ids.insert(r.ids.end(), row.begin(), row.end());
      r.words.insert(r.words.end(), word.begin(), word.end());
    }
  }
  r.off.push_back(r.len.size());
  return r;
}

#define CHECK(c)                                                                      \
  do {                                                                                \
    if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

void check(const dtk_encode_spec &s, const Batch &b) {
  const Rows e = expected(s, b);
  const bool words = (s.flags & DTK_ENC_WORD_IDS) != 0;
  const uint64_t rows = e.len.size();
  for (uint64_t cap : {rows, rows ? rows - 1 : 0}) {
    // (exactly sized, on the heap: new[] of no element is a valid pointer to nothing)
    uint64_t *off = new uint64_t[b.ends.size() + 1], *piece0 = new uint64_t[cap];
    int32_t *ids = new int32_t[cap * s.max_len], *wd = words ? new int32_t[cap * s.max_len] : nullptr;
    uint32_t *len = new uint32_t[cap];
    uint64_t n_rows = ~0ull, n_cut = ~0ull;
    const int rc = dtk_encode_rows_mem(&s, b.piece_off.data(), b.piece_off.size() - 1, b.piece_id.data(), b.ends.data(),
                                       b.ends.size(), b.tok_off.data(), (uint32_t)b.tok_off.size() - 1, cap, off, ids, len,
                                       piece0, wd, &n_rows, &n_cut);
    CHECK(rc == (cap < rows ? DTK_E_CAPACITY : DTK_OK) && n_rows == rows);
    for (size_t u = 0; u <= b.ends.size(); u++) CHECK(off[u] == e.off[u]);
    for (uint64_t r = 0; r < cap; r++) {
      CHECK(len[r] == e.len[r] && piece0[r] == e.piece0[r]);
      for (uint32_t p = 0; p < s.max_len; p++) {
        CHECK(ids[r * s.max_len + p] == e.ids[r * s.max_len + p]);
        if (words) CHECK(wd[r * s.max_len + p] == e.words[r * s.max_len + p]);
      }
    }
    checked += (long)cap;
    delete[] off; delete[] piece0; delete[] ids; delete[] wd; delete[] len;
  }
}
}  // namespace

int main() {
  const int specials[4][2] = {{2, 3}, {2, -1}, {-1, 3}, {-1, -1}};
  for (const auto &sp : specials)
    for (uint32_t first_window = 0; first_window < 2; first_window++) {
      const uint32_t n_special = (sp[0] >= 0) + (sp[1] >= 0);
      for (uint32_t max_len : {1 + n_special, 4u, 5u, 8u}) {
        const uint32_t body = max_len - n_special;
        std::vector<unsigned> ns;
        for (unsigned n = 0; n <= 3 * body; n++) ns.push_back(n);
        ns.insert(ns.end(), {0, 0, body + 1});
        const Batch b = make(ns);
        for (uint32_t stride = 0; stride < body; stride++)
          for (uint32_t words = 0; words < 2; words++)
            check(dtk_encode_spec{max_len, sp[0], sp[1], 1, DTK_ENC_DOCUMENT, stride,
                                  (first_window ? DTK_ENC_FIRST_WINDOW : 0u) | (words ? DTK_ENC_WORD_IDS : 0u)}, b);
      }
    }
  // the argument checks read nothing they should not
  const Batch b = make({3, 0, 7});
  uint64_t off[4], n_rows = 0;
  for (const dtk_encode_spec &bad : {dtk_encode_spec{2, 1, 2, 0, DTK_ENC_DOCUMENT, 0, 0}, dtk_encode_spec{4, 1, 2, 0, DTK_ENC_DOCUMENT, 2, 0},
                                     dtk_encode_spec{65536, 1, 2, 0, DTK_ENC_DOCUMENT, 0, 0}, dtk_encode_spec{4, 1, 2, 0, 2, 0, 0},
                                     dtk_encode_spec{4, 1, 2, 0, DTK_ENC_DOCUMENT, 0, 4}, dtk_encode_spec{4, 1, 2, -1, DTK_ENC_DOCUMENT, 0, 0}})
    CHECK(dtk_encode_rows_mem(&bad, b.piece_off.data(), b.piece_off.size() - 1, b.piece_id.data(), b.ends.data(), b.ends.size(),
                              nullptr, 0, 0, off, nullptr, nullptr, nullptr, nullptr, &n_rows, nullptr) == DTK_E_ARG);
  std::printf("encode_host_check: %ld rows compared, all equal\n", checked);
  return 0;
}
