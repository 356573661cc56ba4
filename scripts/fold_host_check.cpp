// fold_host_check.cpp -- the fold's tables and the WordPiece rule under a fold (datok_amd/csrc/dtk_fold.cpp, dtk_vocab.cpp,
// dtk_fold_core.h, dtk_wordpiece_core.h) in a program of their own, for a run under the host sanitizers.  It makes no HIP
// call and needs no device:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o fold_host_check \
//         scripts/fold_host_check.cpp datok_amd/csrc/dtk_vocab.cpp datok_amd/csrc/dtk_fold.cpp && ./fold_host_check
//
// Every key of the host test's families (tests/fold.py) and a few thousand generated ones are folded through
// dtk_fold_apply_mem and split through dtk_wordpiece_probe_fold_mem, and compared with a plain restatement of the
// definition over std::map; the output arrays are allocated at exactly the needed size, so a byte or a piece written
// behind them is seen, and the keys live in heap blocks of exactly their length, so a byte read behind them is seen.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../datok_amd/csrc/dtk_host.h"

// what dtk_vocab.cpp and dtk_fold.cpp take from the library's other units
DtkDebug g_dbg;
int hip_fail(hipError_t, const char *) { return DTK_E_HIP; }
extern "C" int dtk_device_count(void) { return 0; }

namespace {
using Words = std::vector<std::string>;
using Pieces = std::vector<std::pair<int, unsigned>>;  // (id, end in key bytes)
using Fold = std::map<uint32_t, std::vector<uint32_t>>;

long checked = 0;

std::string utf8(uint32_t cp) {
  std::string s;
  dtk_utf8_put(cp, [&](uint32_t b) { s += (char)b; });
  return s;
}

// the runes of valid UTF-8, by the lead byte alone
std::vector<std::pair<uint32_t, unsigned>> runes_of(const std::string &s) {  // (code point, end)
  std::vector<std::pair<uint32_t, unsigned>> out;
  for (size_t i = 0; i < s.size();) {
    const unsigned c = (unsigned char)s[i], w = c < 0x80 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4;
    uint32_t cp = w == 1 ? c : c & (0x3Fu >> (w - 1));
    for (unsigned k = 1; k < w; k++) cp = (cp << 6) | ((unsigned char)s[i + k] & 0x3Fu);
    i += w;
    out.push_back({cp, (unsigned)i});
  }
  return out;
}

std::string folded(const Fold &f, const std::string &key, unsigned *n_runes = nullptr) {
  std::string out;
  unsigned n = 0;
  for (const auto &r : runes_of(key)) {
    const auto it = f.find(r.first);
    if (it == f.end()) { out += utf8(r.first); n++; continue; }
    for (uint32_t t : it->second) { out += utf8(t); n++; }
  }
  if (n_runes) *n_runes = n;
  return out;
}

// The definition, restated: the largest end on a rune boundary of the key first; an empty fold never matches.
Pieces expected(const Words &words, const Fold &f, const std::string &prefix, int unk, unsigned max_runes, const std::string &key) {
  std::map<std::string, int> d;
  for (size_t i = 0; i < words.size(); i++) d.emplace(words[i], (int)i);
  std::vector<unsigned> ends;
  for (const auto &r : runes_of(key)) ends.push_back(r.second);
  const Pieces unknown = {{unk, (unsigned)key.size()}};
  unsigned n_runes = 0;
  folded(f, key, &n_runes);
  if (n_runes > (max_runes ? max_runes : 100u)) return unknown;
  Pieces out;
  unsigned start = 0;
  while (start < key.size()) {
    bool found = false;
    for (size_t k = ends.size(); k-- > 0 && ends[k] > start;) {
      const std::string c = folded(f, key.substr(start, ends[k] - start));
      if (c.empty()) continue;
      const auto it = d.find((start ? prefix : std::string()) + c);
      if (it == d.end()) continue;
      out.push_back({it->second, ends[k]});
      start = ends[k];
      found = true;
      break;
    }
    if (!found) return unknown;
  }
  return out;
}

struct FoldArrays {
  std::vector<uint32_t> from, to_off, to;
  explicit FoldArrays(const Fold &f) : to_off(1, 0) {
    for (const auto &e : f) {
      from.push_back(e.first);
      to.insert(to.end(), e.second.begin(), e.second.end());
      to_off.push_back((uint32_t)to.size());
    }
  }
};

// the key in a heap block of exactly its length
std::unique_ptr<uint8_t[]> exact(const std::string &key) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[key.size()]);
  if (!key.empty()) memcpy(p.get(), key.data(), key.size());
  return p;
}

void check(const Words &words, const Fold &f, const std::string &prefix, int unk, unsigned max_runes, const std::string &key) {
  const FoldArrays a(f);
  const std::unique_ptr<uint8_t[]> k = exact(key);
  // the folded key, into exactly as many bytes as it has
  const std::string want = folded(f, key);
  std::vector<uint8_t> got(want.size());
  size_t n_bytes = 77;
  int rc = dtk_fold_apply_mem(a.from.data(), a.to_off.data(), a.to.data(), (uint32_t)a.from.size(), k.get(), key.size(), got.data(),
                              got.size(), &n_bytes);
  if (rc != DTK_OK || n_bytes != want.size() || (n_bytes && memcmp(got.data(), want.data(), n_bytes))) {
    fprintf(stderr, "key \"%s\": folded key differs (rc %d, %zu bytes, expected %zu)\n", key.c_str(), rc, n_bytes, want.size());
    exit(1);
  }
  std::string blob;
  std::vector<uint64_t> off(1, 0);
  for (const std::string &w : words) { blob += w; off.push_back(blob.size()); }
  const Pieces exp = expected(words, f, prefix, unk, max_runes, key);
  const auto probe = [&](int32_t *ids, uint32_t *ends, uint32_t cap, uint32_t *n) {
    return dtk_wordpiece_probe_fold_mem(reinterpret_cast<const uint8_t *>(blob.data()), off.data(), (uint32_t)words.size(),
                                        reinterpret_cast<const uint8_t *>(prefix.data()), (uint32_t)prefix.size(), unk, max_runes,
                                        a.from.data(), a.to_off.data(), a.to.data(), (uint32_t)a.from.size(), k.get(), key.size(),
                                        ids, ends, cap, n);
  };
  uint32_t n = 77;
  rc = probe(nullptr, nullptr, 0, &n);  // the count alone
  if (rc != (exp.empty() ? DTK_OK : DTK_E_CAPACITY) || n != exp.size()) {
    fprintf(stderr, "key \"%s\": count %u (rc %d), expected %zu\n", key.c_str(), n, rc, exp.size());
    exit(1);
  }
  std::vector<int32_t> ids(exp.size());    // exactly as many as needed: one write too many is a heap overflow
  std::vector<uint32_t> ends(exp.size());
  if (!exp.empty() && ((rc = probe(ids.data(), ends.data(), (uint32_t)exp.size(), &n)) != DTK_OK || n != exp.size())) {
    fprintf(stderr, "key \"%s\": rc %d, %u pieces\n", key.c_str(), rc, n);
    exit(1);
  }
  for (size_t i = 0; i < exp.size(); i++)
    if (ids[i] != exp[i].first || ends[i] != exp[i].second) {
      fprintf(stderr, "key \"%s\", piece %zu: got (%d, %u), expected (%d, %u)\n", key.c_str(), i, ids[i], ends[i], exp[i].first,
              exp[i].second);
      exit(1);
    }
  checked++;
}

const std::string R = "\xef\xbf\xbd";
}  // namespace

int main() {
  // the hand-written mapping of tests/fold.py
  Fold hand;
  for (uint32_t c = 'A'; c <= 'Z'; c++) hand[c] = {c + 32};
  hand[0xC4] = {'a'}; hand[0xD6] = {'o'}; hand[0xDC] = {'u'}; hand[0xE4] = {'a'}; hand[0xF6] = {'o'}; hand[0xFC] = {'u'};
  hand[0xC9] = {'e'}; hand[0xE9] = {'e'};
  hand[0xD55C] = {0x1112, 0x1161, 0x11AB};
  hand[0x10400] = {0x10428};
  hand[0x09CB] = {0x09C7, 0x09BE};
  hand[0x0301] = {}; hand[0x0308] = {};
  Fold hand_r = hand;
  hand_r[0xFFFD] = {};
  const std::string UE = utf8(0xDC), AE = utf8(0xC4), ACUTE = utf8(0x301), DIA = utf8(0x308), HANGUL = utf8(0xD55C),
                    JAMO = utf8(0x1112) + utf8(0x1161) + utf8(0x11AB), DES = utf8(0x10400), des = utf8(0x10428),
                    KA = utf8(0x995), O = utf8(0x9CB), E = utf8(0x9C7), AA = utf8(0x9BE);
  std::string long_key = std::string(50, 'a') + ACUTE + std::string(49, 'a') + DIA;
  struct Family { const Fold *f; Words words; Words keys; };
  const std::vector<Family> families = {
      {&hand, {"[UNK]", "uber"}, {UE + "ber", "UBER", UE + "bel", "", "u"}},
      {&hand, {"[UNK]", "aaaa"}, {AE + AE + AE + AE, AE + AE + AE + AE + AE, AE}},
      {&hand, {"[UNK]", "ab", "##c", utf8(0x1112)}, {HANGUL, "ab" + HANGUL, HANGUL + HANGUL}},
      {&hand, {"[UNK]", JAMO, "ab", "##" + JAMO}, {HANGUL, "ab" + HANGUL, HANGUL + HANGUL}},
      {&hand, {"[UNK]", des, "##" + des}, {DES, DES + des, des + DES + "x"}},
      {&hand, {"[UNK]", KA + E + AA, KA, E, "##" + E, "##" + AA}, {KA + O, KA + KA + O, O}},
      {&hand, {"[UNK]", "", "##", "a", "##b"}, {"a" + ACUTE + "b", "a" + ACUTE, ACUTE + "a", ACUTE, "a" + ACUTE + DIA + "b" + ACUTE,
                                               ACUTE + DIA, AE + "b", "ab" + ACUTE + "c", "b" + ACUTE}},
      {&hand_r, {"[UNK]", "ab", "##cd"}, {"ab" + R + "cd", R, R + "ab", "ab" + R}},
      {&hand, {"[UNK]", "ab", "##cd", "##" + R}, {"AB" + R + "cd", R}},
      {&hand, {"[UNK]", "x", "##y", "x", "##y"}, {"XY", "xyY"}},
      {&hand, {"[UNK]", "ab", "##ab", "cd"}, {"ABAB", "ABCD"}},
      {&hand, {"[UNK]", "a", "##a"}, {long_key, std::string(101, 'A'), std::string(100, 'A')}},
  };
  const Fold none;
  for (int bits : {-1, 0, 2}) {
    g_dbg.vocab_hash_bits = bits;
    for (const Family &f : families)
      for (const std::string &k : f.keys)
        for (unsigned max_runes : {0u, 1u, 3u}) {
          check(f.words, *f.f, "##", 0, max_runes, k);
          check(f.words, none, "##", 0, max_runes, k);  // (the empty mapping: the unfolded rule)
        }
    // generated keys whose letters shrink, grow, vanish and double; words of one or two folded letters
    const std::vector<std::string> letters = {"a", "b", "A", "B", AE, UE, ACUTE, DIA, HANGUL, DES, O, "\xe2\x82\xac"};
    const std::vector<std::string> low = {"a", "b", "u", JAMO, des, E + AA, E, "\xe2\x82\xac"};
    uint32_t seed = 4711u + (uint32_t)bits;
    const auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
    const auto word = [&](const std::vector<std::string> &from, uint32_t lo, uint32_t hi) {
      std::string s;
      for (uint32_t n = lo + rnd(hi - lo + 1); n > 0; n--) s += from[rnd((uint32_t)from.size())];
      return s;
    };
    for (int round = 0; round < 40; round++) {
      Words words = {"<unk>"};
      for (uint32_t n = 4 + rnd(20); n > 0; n--) words.push_back(word(low, 1, 2));
      for (uint32_t n = 4 + rnd(30); n > 0; n--) words.push_back("##" + word(low, 1, 2));
      const int unk = (int)rnd((uint32_t)words.size());
      for (int k = 0; k < 12; k++) check(words, hand, "##", unk, k % 3 ? 0u : 5u, word(letters, 1, 8));
    }
  }
  g_dbg.vocab_hash_bits = -1;
  // bytes that do not decode, at the very end of their block too: one U+FFFD each
  const FoldArrays a(hand_r), b(hand);
  for (const std::string &key : {std::string("ab\xff" "cd"), std::string("\xe2\x82"), std::string("x\xc3"), std::string("\xf0\x9f\x98"),
                                 std::string("\xed\xa0\x80"), std::string("\xf4\x90\x80\x80"), std::string("\x80"), std::string("A\xd0")}) {
    const std::unique_ptr<uint8_t[]> k = exact(key);
    uint8_t out[64];
    size_t n = 0, m = 0;
    if (dtk_fold_apply_mem(a.from.data(), a.to_off.data(), a.to.data(), (uint32_t)a.from.size(), k.get(), key.size(), out, 64, &n) != DTK_OK ||
        dtk_fold_apply_mem(b.from.data(), b.to_off.data(), b.to.data(), (uint32_t)b.from.size(), k.get(), key.size(), out, 64, &m) != DTK_OK) {
      fprintf(stderr, "invalid bytes refused\n");
      return 1;
    }
    size_t bad = 0, ascii = 0;
    for (unsigned char c : key) { bad += c >= 0x80; ascii += c < 0x80; }
    if (n != ascii || m != ascii + 3 * bad) { fprintf(stderr, "invalid bytes: %zu and %zu bytes\n", n, m); return 1; }
    int32_t ids[4];
    uint32_t ends[4], np = 0;
    const uint8_t blob[1] = {'a'};
    const uint64_t off[2] = {0, 1};
    if (dtk_wordpiece_probe_fold_mem(blob, off, 1, blob, 0, 0, 0, b.from.data(), b.to_off.data(), b.to.data(), (uint32_t)b.from.size(),
                                     k.get(), key.size(), ids, ends, 4, &np) != DTK_E_ARG) {
      fprintf(stderr, "the probe took a key that is no UTF-8\n");
      return 1;
    }
    checked++;
  }
  // folds outside their ranges are refused before anything is read
  uint8_t out[8];
  size_t n = 0;
  const auto apply = [&](std::vector<uint32_t> from, std::vector<uint32_t> to_off, std::vector<uint32_t> to) {
    return dtk_fold_apply_mem(from.data(), to_off.data(), to.data(), (uint32_t)from.size(), out, 0, out, 8, &n);
  };
  if (apply({0x61}, {0, 1}, {0x62}) != DTK_OK || apply({0xD800}, {0, 1}, {0x62}) != DTK_E_ARG || apply({0x110000}, {0, 1}, {0x62}) != DTK_E_ARG ||
      apply({0x61, 0x61}, {0, 1, 2}, {0x62, 0x63}) != DTK_E_ARG || apply({0x61}, {0, 5}, {1, 2, 3, 4, 5}) != DTK_E_ARG ||
      apply({0x61}, {0, 1}, {0x110000}) != DTK_E_ARG || apply({0x61}, {0, 1}, {0xDC00}) != DTK_E_ARG ||
      apply({0x61, 0x62}, {1, 1, 2}, {0x62, 0x63}) != DTK_E_ARG || apply({0x61, 0x62}, {0, 2, 1}, {0x62, 0x63}) != DTK_E_ARG) {
    fprintf(stderr, "bad fold arguments accepted\n");
    return 1;
  }
  printf("fold_host_check: %ld keys agree\n", checked);
  return 0;
}
