// The host functions of interaction constraints (csrc/grow.hpp, grow.cpp) in a program of their own, for a build with
// -fsanitize=address,undefined (CPU only; tests/test_grow_interact_cpu.py builds and runs it): the grammar of
// "ohx_interaction_constraints" on values held in buffers of exactly their length, a refused value leaving the caller's
// groups, whether groups are active, and grow_interact_allowed against sets made one feature at a time, with ids at the
// word boundary and with 64 groups.  Exits 0 and prints "0 failures" when every invariant holds.
// usage: grow_interact_host_check [draws] [seed]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "grow.hpp"

using namespace ohx;

static long failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      ++failures;                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);            \
    }                                                            \
  } while (0)

static long values = 0, sets = 0;

// the parser on a copy of `s` that ends with the terminator and nothing after it
static bool parse(const std::string& s, std::vector<uint64_t>* out) {
  std::unique_ptr<char[]> exact(new char[s.size() + 1]);
  memcpy(exact.get(), s.c_str(), s.size() + 1);
  ++values;
  return grow_interact_parse(exact.get(), out);
}

static std::set<uint32_t> members(const uint64_t w[2]) {
  std::set<uint32_t> m;
  for (uint32_t f = 0; f < kGrowMaxFeatures; ++f)
    if (grow_interact_has(w, f)) m.insert(f);
  return m;
}

static std::string text(const std::vector<std::vector<uint32_t>>& groups, const char* sep) {
  std::string s = "[";
  for (size_t g = 0; g < groups.size(); ++g) {
    s += g ? std::string(",") + sep + "[" : std::string("[");
    for (size_t k = 0; k < groups[g].size(); ++k) s += (k ? std::string(",") + sep : std::string()) + std::to_string(groups[g][k]);
    s += "]";
  }
  return s + "]";
}

static void check_grammar() {
  std::vector<uint64_t> w{7, 7};
  EXPECT(parse("[]", &w) && w.empty());
  EXPECT(parse(" [ ] ", &w) && w.empty());
  EXPECT(parse("[[0, 2], [1, 3, 4]]", &w) && w.size() == 4 && w[0] == 5 && w[1] == 0 && w[2] == 26 && w[3] == 0);
  EXPECT(parse("[[63,64,127]]", &w) && w.size() == 2 && w[0] == 1ull << 63 && w[1] == (1ull | 1ull << 63));
  EXPECT(parse("\t[\t[ 007 ]\t]\t", &w) && w.size() == 2 && w[0] == 128);
  EXPECT(parse("[[1],[1],[1,2]]", &w) && w.size() == 6);   // a feature in several groups, and a group twice
  const std::vector<uint64_t> kept = w;
  for (const char* bad : {"", " ", "[", "]", "[[]]", "[0, 1]", "[[0, 0]]", "[[1.0]]", "[[-1]]", "[[+1]]", "[[0],]", "[[0,]]", "[,[0]]", "[[0]],",
                          "[[0]] x", "[[0] [1]]", "[[0 1]]", "[[128]]", "[[4294967296]]", "[[99999999999999999999]]", "[[0]", "[[0", "[[0,", "((0))",
                          "[[0]]]", "[[[0]]]", "[[1e1]]", "[[0x1]]"}) {
    EXPECT(!parse(bad, &w));
    EXPECT(w == kept);   // a refused value leaves the previous one
  }
  EXPECT(!grow_interact_parse(nullptr, &w) && !grow_interact_parse("[]", nullptr));
  std::vector<std::vector<uint32_t>> many;
  for (uint32_t g = 0; g < kGrowMaxGroups; ++g) many.push_back({g, g + 64});
  EXPECT(parse(text(many, " "), &w) && w.size() == 2 * kGrowMaxGroups && w[2 * 63] == 1ull << 63 && w[2 * 63 + 1] == 1ull << 63);
  many.push_back({0});
  EXPECT(!parse(text(many, ""), &w) && w.size() == 2 * kGrowMaxGroups);
}

static void check_active() {
  std::vector<uint64_t> w;
  EXPECT(!grow_interact_active(nullptr, 0, 6));
  EXPECT(parse("[[0,1,2],[3,4,5]]", &w) && grow_interact_active(w.data(), 2, 6) && !grow_interact_active(w.data(), 2, 3));
  EXPECT(parse("[[0,1],[5,4,3,2,1,0]]", &w) && !grow_interact_active(w.data(), 2, 6) && grow_interact_active(w.data(), 2, 7));
  uint64_t all[2];
  grow_interact_all(128, all);
  EXPECT(all[0] == ~0ull && all[1] == ~0ull && !grow_interact_active(all, 1, 128));
  grow_interact_all(64, all);
  EXPECT(all[0] == ~0ull && all[1] == 0 && !grow_interact_active(all, 1, 64) && grow_interact_active(all, 1, 65));
  grow_interact_all(65, all);
  EXPECT(all[0] == ~0ull && all[1] == 1);
  grow_interact_all(1, all);
  EXPECT(all[0] == 1 && all[1] == 0);
  grow_interact_all(127, all);
  EXPECT(all[1] == ~0ull >> 1);
}

static void check_allowed(int draws, uint64_t seed0) {
  std::mt19937_64 rng(seed0);
  for (int it = 0; it < draws; ++it) {
    const uint32_t F = it % 7 == 0 ? kGrowMaxFeatures : 1 + (uint32_t)(rng() % kGrowMaxFeatures);
    const uint32_t ngroups = it % 11 == 0 ? kGrowMaxGroups : (uint32_t)(rng() % (kGrowMaxGroups + 1));
    std::vector<std::set<uint32_t>> groups(ngroups);
    std::vector<std::vector<uint32_t>> lists(ngroups);
    for (uint32_t g = 0; g < ngroups; ++g) {
      // (ids about the word boundary in every fifth draw: the group is no larger than the ids it draws from)
      const bool boundary = it % 5 == 0 && F > 64;
      const uint32_t first = boundary ? 60 : 0, span = boundary ? std::min<uint32_t>(F - 60, 8) : F;
      const uint32_t size = 1 + (uint32_t)(rng() % std::min<uint32_t>(span, 9));
      while (groups[g].size() < size) groups[g].insert(first + (uint32_t)(rng() % span));
      lists[g].assign(groups[g].begin(), groups[g].end());
      std::shuffle(lists[g].begin(), lists[g].end(), rng);
    }
    // the words in a buffer of exactly their size, by the parser
    std::vector<uint64_t> parsed;
    EXPECT(parse(text(lists, it % 2 ? " " : ""), &parsed) && parsed.size() == 2 * (size_t)ngroups);
    std::unique_ptr<uint64_t[]> words(new uint64_t[2 * (size_t)ngroups + (ngroups ? 0 : 1)]);
    std::copy(parsed.begin(), parsed.end(), words.get());
    for (uint32_t g = 0; g < ngroups; ++g) EXPECT(members(words.get() + 2 * g) == groups[g]);
    // a path: nothing, one feature, or some features of a group, or any features
    std::set<uint32_t> path;
    const int kind = it % 4;
    if (kind == 1) path.insert((uint32_t)(rng() % F));
    if (kind == 2 && ngroups)
      for (uint32_t f : groups[rng() % ngroups])
        if (rng() % 2) path.insert(f);
    if (kind == 3)
      for (int k = 0; k < 3; ++k) path.insert((uint32_t)(rng() % F));
    uint64_t P[2] = {0, 0}, A[2] = {~0ull, ~0ull};
    for (uint32_t f : path) P[f >> 6] |= 1ull << (f & 63);
    grow_interact_allowed(P, words.get(), ngroups, F, A);
    std::set<uint32_t> want;
    if (path.empty()) {
      for (uint32_t f = 0; f < F; ++f) want.insert(f);
    } else {
      want = path;
      for (const auto& g : groups)
        if (std::includes(g.begin(), g.end(), path.begin(), path.end())) want.insert(g.begin(), g.end());
    }
    EXPECT(members(A) == want);
    ++sets;
  }
}

int main(int argc, char** argv) {
  const int draws = argc > 1 ? atoi(argv[1]) : 3000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 35;
  check_grammar();
  check_active();
  check_allowed(draws, seed);
  printf("%ld values, %ld sets, %ld failures\n", values, sets, failures);
  return failures == 0 ? 0 : 1;
}
