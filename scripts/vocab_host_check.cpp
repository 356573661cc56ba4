// vocab_host_check.cpp -- the vocabulary table's builder and probe (datok_amd/csrc/dtk_vocab.cpp, dtk_vocab_core.h) in a
// program of their own, for a run under the host sanitizers.  It makes no HIP call and needs no device:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -o vocab_host_check \
//         scripts/vocab_host_check.cpp datok_amd/csrc/dtk_vocab.cpp && ./vocab_host_check
//
// Every key of the host test's vocabularies (tests/test_token_ids_host.py) is looked up through dtk_vocab_probe_mem and
// compared with a std::map that keeps the lowest index, with the whole hash and with 0, 1 and 2 bits of it.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../datok_amd/csrc/dtk_host.h"

// what dtk_vocab.cpp takes from the library's other units
DtkDebug g_dbg;
int hip_fail(hipError_t, const char *) { return DTK_E_HIP; }
extern "C" int dtk_device_count(void) { return 0; }

namespace {
using Words = std::vector<std::string>;

long checked = 0;

int probe(const Words &words, const std::string &key) {
  std::string blob;
  std::vector<uint64_t> off(1, 0);
  for (const std::string &w : words) { blob += w; off.push_back(blob.size()); }
  int32_t id = 7;
  const int rc = dtk_vocab_probe_mem(reinterpret_cast<const uint8_t *>(blob.data()), off.data(), (uint32_t)words.size(),
                                     reinterpret_cast<const uint8_t *>(key.data()), key.size(), &id);
  if (rc != DTK_OK) { fprintf(stderr, "dtk_vocab_probe_mem: %d\n", rc); exit(2); }
  return id;
}

void check(const Words &words, const Words &keys, int bits) {
  std::map<std::string, int> want;
  for (size_t i = 0; i < words.size(); i++) want.emplace(words[i], (int)i);  // (emplace keeps the first: the lowest index)
  g_dbg.vocab_hash_bits = bits;
  for (const std::string &k : keys) {
    const auto it = want.find(k);
    const int exp = it == want.end() ? -1 : it->second, got = probe(words, k);
    if (got != exp) {
      fprintf(stderr, "bits %d, %zu words, key \"%s\": got %d, expected %d\n", bits, words.size(), k.c_str(), got, exp);
      exit(1);
    }
    checked++;
  }
  g_dbg.vocab_hash_bits = -1;
}

Words with_neighbours(const Words &words, size_t step) {
  Words keys;
  for (size_t i = 0; i < words.size(); i += step) {
    const std::string &w = words[i];
    keys.push_back(w);
    keys.push_back(w + "!");
    keys.push_back("!" + w);
    if (!w.empty()) {
      keys.push_back(w.substr(0, w.size() - 1));
      keys.push_back(w.substr(1));
      std::string x = w;
      x.back() ^= 1;
      keys.push_back(x);
    }
  }
  keys.push_back("");
  keys.push_back(std::string(1, '\0'));
  return keys;
}
}  // namespace

int main() {
  for (int bits : {-1, 0, 1, 2}) {
    for (int n : {0, 1, 2, 3, 5, 1000}) {
      Words words;
      for (int i = 0; i < n; i++) words.push_back("w" + std::to_string(i));
      check(words, with_neighbours(words, n < 1000 || bits < 0 ? 1 : 97), bits);
    }
    Words fam = {"a", "ab", "abc", "abcd", "abcde", "abcdefgh", "abcdefghi", "Worta", "Wortb", "Wortc", "Wortx", "Worty", "Wortz",
                 std::string(17, 'x') + "0", std::string(17, 'x') + "1", "", std::string(1, '\0'), std::string(2, '\0'),
                 "\xef\xbf\xbd", "\xff", "Gr\xc3\xbc\xc3\x9f" "e"};
    check(fam, with_neighbours(fam, 1), bits);
    Words dup = {"der", "die", "der", "", "das", "die", "", "der"};
    check(dup, with_neighbours(dup, 1), bits);
    Words lng = {std::string(3000, 'q') + "a", std::string(3000, 'q') + "b", std::string(3000, 'q')};
    check(lng, with_neighbours(lng, 1), bits);
  }
  // offsets that do not ascend, do not begin at 0 or pass 2^32 are refused before anything is read
  const uint8_t blob[3] = {'a', 'b', 'x'};
  int32_t id = 0;
  const uint64_t down[3] = {0, 3, 2}, late[3] = {1, 2, 3}, huge[3] = {0, 2, 1ull << 32};
  for (const uint64_t *off : {down, late, huge})
    if (dtk_vocab_probe_mem(blob, off, 2, blob, 1, &id) != DTK_E_ARG) { fprintf(stderr, "bad offsets accepted\n"); return 1; }
  dtk_vocab *v = nullptr;
  const uint64_t ok[3] = {0, 2, 3};
  if (dtk_vocab_create(blob, ok, 2, &v) != DTK_E_NO_DEVICE || v) { fprintf(stderr, "dtk_vocab_create without a device\n"); return 1; }
  printf("vocab_host_check: %ld lookups agree\n", checked);
  return 0;
}
