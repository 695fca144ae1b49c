// tests/check_net_variants.cpp — the kP2PNet flag sets (ggrs_amd/csrc/p2p_variant.hpp) the rows of
// tests/test_p2p_net_matrix.py launch.  Every argument is one launch,
//   game:T:W:sparse:fanout:generic:K:log:desync:peer
// (game one of the trait sets below; the rest P2PLaunchFacts), answered by a line "chosen <flag set>"
// from p2p_choose.  Before them, per trait set: "reachable", the kP2PNet flag sets
// p2p_variant_reachable allows, and "choosable", those p2p_choose returns for some launch (every
// combination of launch facts, as tests/check_p2p_variant.cpp walks them).  No GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "p2p_variant.hpp"

namespace {
using namespace rb;

// the trait sets of tests/check_p2p_variant.cpp (games.hpp: lanes, players, input bytes, NWL,
// sizeof(CS), alphabet, fan-out, in-lane fan-out)
struct Game {
  const char* name;
  P2PTraits t;
};
const Game kGames[] = {
    {"ex2", {2, 2, 1, 5, 2, 16u, true, true}},
    {"ex4", {4, 4, 1, 5, 2, 16u, true, true}},
    {"brawler", {64, 2, 1, 32, 2, 256u, true, false}},
    {"stub", {1, 2, 4, 1, 8, 0xFFFFFFFFu, false, false}},
};

std::string name_of(uint32_t v) {
  static const struct {
    uint32_t bit;
    const char* name;
  } kNames[] = {{kP2PNet, "Net"},     {kP2PSparse, "Sparse"}, {kP2PSpec, "Spec"}, {kP2PMtf, "Mtf"}, {kP2PLdsC, "LdsC"},
                {kP2PAsync, "Async"}, {kP2PWire, "Wire"},     {kP2PQ, "Q"},       {kP2POne, "One"}, {kP2PLog, "Log"}};
  std::string s;
  for (const auto& n : kNames)
    if (v & n.bit) s += (s.empty() ? "" : "|") + std::string(n.name);
  return s.empty() ? "plain" : s;
}

void print_set(const char* what, const char* game, const std::set<uint32_t>& vs) {
  std::printf("%s %s", what, game);
  for (uint32_t v : vs) std::printf(" %s", name_of(v).c_str());
  std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  for (const Game& g : kGames) {
    std::set<uint32_t> reachable, choosable;
    for (uint32_t v = 0; v < kP2PVariants; ++v)
      if ((v & kP2PNet) && p2p_variant_reachable(g.t, v)) reachable.insert(v);
    const int Ts[] = {1, 2, 3, 4, 23, 24, 50}, Ws[] = {8, 9}, Ks[] = {8, 16};
    for (int T : Ts)
      for (int W : Ws)
        for (int K : Ks)
          for (unsigned b = 0; b < (1u << 9); ++b) {
            const P2PLaunchFacts f{T, W, 256, (b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, K,
                                   (b & 16) != 0, (b & 32) != 0, (b & 64) != 0, (b & 128) != 0, (b & 256) != 0};
            const uint32_t v = p2p_choose(g.t, f).variant;
            if (v & kP2PNet) choosable.insert(v);
          }
    print_set("reachable", g.name, reachable);
    print_set("choosable", g.name, choosable);
  }
  for (int i = 1; i < argc; ++i) {
    char game[16];
    int T, W, sparse, spec, generic, K, log, ds, peer;
    if (std::sscanf(argv[i], "%15[^:]:%d:%d:%d:%d:%d:%d:%d:%d:%d", game, &T, &W, &sparse, &spec, &generic, &K, &log, &ds,
                    &peer) != 10) {
      std::printf("bad argument %s\n", argv[i]);
      return 2;
    }
    const Game* g = nullptr;
    for (const Game& k : kGames)
      if (std::strcmp(k.name, game) == 0) g = &k;
    if (!g) {
      std::printf("unknown game %s\n", game);
      return 2;
    }
    // a test-sized batch: block 256, lane-asynchronous ticks allowed, at most two waves per SIMD, no packets
    const P2PLaunchFacts f{T, W, 256, false, sparse != 0, spec != 0, generic != 0, K, false, false, log != 0, ds != 0, peer != 0};
    const P2PChoice c = p2p_choose(g->t, f);
    if (!p2p_variant_reachable(g->t, c.variant)) {
      std::printf("%s: p2p_choose returned 0x%x, which the game does not instantiate\n", argv[i], c.variant);
      return 1;
    }
    std::printf("chosen %s\n", name_of(c.variant).c_str());
  }
  return 0;
}
