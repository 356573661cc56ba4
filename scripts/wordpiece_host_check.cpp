// wordpiece_host_check.cpp -- the vocabulary builder and the WordPiece rule (datok_amd/csrc/dtk_vocab.cpp,
// dtk_wordpiece_core.h) in a program of their own, for a run under the host sanitizers.  It makes no HIP call and needs
// no device:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o wordpiece_host_check \
//         scripts/wordpiece_host_check.cpp datok_amd/csrc/dtk_vocab.cpp && ./wordpiece_host_check
//
// Every key of the host test's word families (tests/wordpiece.py) and a few thousand generated ones are split through
// dtk_wordpiece_probe_mem and compared with a plain restatement of the definition over a std::map that keeps the lowest
// index, with the whole hash and with 0, 1 and 2 bits of it; the output arrays are allocated at exactly the needed
// size, so a piece written behind them is seen.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../datok_amd/csrc/dtk_host.h"

// what dtk_vocab.cpp takes from the library's other units
DtkDebug g_dbg;
int hip_fail(hipError_t, const char *) { return DTK_E_HIP; }
extern "C" int dtk_device_count(void) { return 0; }

namespace {
using Words = std::vector<std::string>;
using Pieces = std::vector<std::pair<int, unsigned>>;  // (id, end in key bytes)

long checked = 0;

// The definition, restated: the largest end on a rune boundary first.
Pieces expected(const Words &words, const std::string &prefix, int unk, unsigned max_runes, const std::string &key) {
  std::map<std::string, int> d;
  for (size_t i = 0; i < words.size(); i++) d.emplace(words[i], (int)i);
  std::vector<unsigned> ends;
  for (unsigned e = 1; e <= key.size(); e++)
    if (e == key.size() || ((unsigned char)key[e] & 0xC0) != 0x80) ends.push_back(e);
  const Pieces unknown = {{unk, (unsigned)key.size()}};
  if (ends.size() > (max_runes ? max_runes : 100u)) return unknown;
  Pieces out;
  unsigned start = 0;
  while (start < key.size()) {
    bool found = false;
    for (size_t k = ends.size(); k-- > 0 && ends[k] > start;) {
      const auto it = d.find((start ? prefix : std::string()) + key.substr(start, ends[k] - start));
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

void check(const Words &words, const std::string &prefix, int unk, unsigned max_runes, const std::string &key) {
  std::string blob;
  std::vector<uint64_t> off(1, 0);
  for (const std::string &w : words) { blob += w; off.push_back(blob.size()); }
  const Pieces exp = expected(words, prefix, unk, max_runes, key);
  const auto probe = [&](int32_t *ids, uint32_t *ends, uint32_t cap, uint32_t *n) {
    return dtk_wordpiece_probe_mem(reinterpret_cast<const uint8_t *>(blob.data()), off.data(), (uint32_t)words.size(),
                                   reinterpret_cast<const uint8_t *>(prefix.data()), (uint32_t)prefix.size(), unk, max_runes,
                                   reinterpret_cast<const uint8_t *>(key.data()), key.size(), ids, ends, cap, n);
  };
  uint32_t n = 77;
  int rc = probe(nullptr, nullptr, 0, &n);  // the count alone
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
  for (size_t k = 0; k < exp.size(); k++)
    if (ids[k] != exp[k].first || ends[k] != exp[k].second) {
      fprintf(stderr, "key \"%s\", piece %zu: got (%d, %u), expected (%d, %u)\n", key.c_str(), k, ids[k], ends[k], exp[k].first,
              exp[k].second);
      exit(1);
    }
  checked++;
}

const std::string R = "\xef\xbf\xbd";
}  // namespace

int main() {
  struct Family { Words words; std::string prefix; Words keys; };
  const std::vector<Family> families = {
      {{"[UNK]", "un", "##aff", "##able"}, "##", {"unaffable", "unaffablex", "un", "aff", "", "u", "unaff", "unable"}},
      {{"[UNK]", "ab", "abc", "##cd"}, "##", {"abcd", "abc", "ab", "abcdcd"}},
      {{"[UNK]", "a", "ab", "abc", "##c", "##d"}, "##", {"abcd", "abc", "abd", "ad", "acd", "adc"}},
      {{"[UNK]", "ab", "cd"}, "##", {"abcd", "ab", "cd"}},
      {{"[UNK]", "ab", "##cd"}, "##", {"abcd", "cd"}},
      {{"[UNK]", "ab", "cd"}, "", {"abcd", "cdab", "abab", "abc"}},
      {{"[UNK]", "\xc3", "##\x9f", "Stra", "##\xc3", "##\x9f"}, "##", {"Stra\xc3\x9f", "Stra"}},
      {{"[UNK]", "\xc3", "##\x9f", "Stra", "##\xc3", "##\x9f", "##\xc3\x9f"}, "##", {"Stra\xc3\x9f", "Stra\xc3\x9f\xc3\x9f"}},
      {{"[UNK]", "ab", "##" + R, "##cd", R}, "##", {"ab" + R + "cd", R + R, "ab" + R + "x", R, "ab" + R}},
      {{"[UNK]", "", "##", "a", "##b"}, "##", {"ab", "ac", "", "a", "b"}},
      {{"[UNK]", "x", "##y", "x", "##y", "[UNK]"}, "##", {"xy", "xyy", "[UNK]", "y"}},
      {{"[UNK]", "a", "0123456789abcdefb"}, "0123456789abcdef", {"ab", "abb", "b"}},
  };
  for (int bits : {-1, 0, 1, 2}) {
    g_dbg.vocab_hash_bits = bits;
    for (const Family &f : families)
      for (const std::string &k : f.keys)
        for (unsigned max_runes : {0u, 1u, 3u}) check(f.words, f.prefix, 0, max_runes, k);
    // generated keys over a small alphabet with letters of 1 to 4 bytes, words of one or two letters
    const std::vector<std::string> letters = {"a", "b", "c", "\xc3\xa4", "\xe2\x82\xac", "\xf0\x90\x8c\xb0"};
    uint32_t seed = 12345u + (uint32_t)bits;
    const auto rnd = [&](uint32_t n) { seed = seed * 1664525u + 1013904223u; return (seed >> 8) % n; };
    const auto word = [&](uint32_t lo, uint32_t hi) {
      std::string s;
      for (uint32_t n = lo + rnd(hi - lo + 1); n > 0; n--) s += letters[rnd((uint32_t)letters.size())];
      return s;
    };
    for (int round = 0; round < 40; round++) {
      Words words = {"<unk>"};
      for (uint32_t n = 4 + rnd(20); n > 0; n--) words.push_back(word(1, 2));
      for (uint32_t n = 4 + rnd(30); n > 0; n--) words.push_back("##" + word(1, 2));
      const int unk = (int)rnd((uint32_t)words.size());
      for (int k = 0; k < 12; k++) check(words, "##", unk, k % 3 ? 0u : 5u, word(1, 8));
    }
    // the default of 100 runes, at its edge, with letters of one and of two bytes
    const Words aa = {"[UNK]", "a", "##a", "\xc3\xa4", "##\xc3\xa4"};
    for (size_t n : {99u, 100u, 101u}) {
      check(aa, "##", 0, 0, std::string(n, 'a'));
      std::string u;
      for (size_t i = 0; i < n; i++) u += "\xc3\xa4";
      check(aa, "##", 0, 0, u);
      check(aa, "##", 0, 101, u);
    }
  }
  g_dbg.vocab_hash_bits = -1;
  // arguments outside their ranges are refused before anything is read
  const uint8_t blob[4] = {'a', '#', '#', 'b'};
  const uint64_t off[3] = {0, 1, 4}, down[3] = {0, 3, 2};
  const uint8_t pre[17] = {'#', '#'};
  int32_t ids[4];
  uint32_t ends[4], n = 0;
  const auto call = [&](const uint64_t *o, const uint8_t *p, uint32_t pl, int32_t unk, uint32_t *np) {
    return dtk_wordpiece_probe_mem(blob, o, 2, p, pl, unk, 0, blob, 1, ids, ends, 4, np);
  };
  if (call(off, pre, 2, 0, &n) != DTK_OK || n != 1 || ids[0] != 0 || ends[0] != 1) { fprintf(stderr, "plain call\n"); return 1; }
  if (call(down, pre, 2, 0, &n) != DTK_E_ARG || call(off, pre, 17, 0, &n) != DTK_E_ARG || call(off, nullptr, 2, 0, &n) != DTK_E_ARG ||
      call(off, pre, 2, 2, &n) != DTK_E_ARG || call(off, pre, 2, -1, &n) != DTK_E_ARG || call(off, pre, 2, 0, nullptr) != DTK_E_ARG) {
    fprintf(stderr, "bad arguments accepted\n");
    return 1;
  }
  printf("wordpiece_host_check: %ld splits agree\n", checked);
  return 0;
}
