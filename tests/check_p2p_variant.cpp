// tests/check_p2p_variant.cpp — p2p_choose (ggrs_amd/csrc/p2p_variant.hpp) against the rule it
// replaced: GameOpsT::launch_p2p and its nested launch_p2p_as / _as_l / _as_m of commit bc5fca4,
// transcribed below as the nested ifs they were (each `if constexpr` on the game an `if` on the
// traits, each launch a returned flag set and LDS size), over every combination of launch facts.
// tests/test_p2p_variant.py compiles and runs it; no GPU.
#include <cstdio>
#include <set>

#include "p2p_variant.hpp"

namespace {
using namespace rb;

struct Ref {
  uint32_t v;
  size_t lds;
  bool set_attr;  // the launch called hipFuncSetAttribute for its LDS size
};
uint32_t flags(bool spec, bool sparse, bool net, bool ldsc, bool async, bool wire = false, bool mtf = false, bool q = false,
               bool one = false, bool log = false) {
  return (spec ? kP2PSpec : 0u) | (sparse ? kP2PSparse : 0u) | (net ? kP2PNet : 0u) | (ldsc ? kP2PLdsC : 0u) |
         (async ? kP2PAsync : 0u) | (wire ? kP2PWire : 0u) | (mtf ? kP2PMtf : 0u) | (q ? kP2PQ : 0u) | (one ? kP2POne : 0u) |
         (log ? kP2PLog : 0u);
}

// ---- p2p.hpp at bc5fca4, the product's constants as numbers
bool ref_lds_queue(const P2PTraits& g) { return g.input_bytes == 1 && (g.lanes > 1 || g.players == 1); }
size_t ref_lds_bytes(const P2PTraits& g, bool ldsc, int block) {
  return ref_lds_queue(g) && (ldsc || !1 /* RB_SHORT_HBM_RING */) ? size_t{128} * static_cast<size_t>(block) : 0;
}
size_t ref_lds_cell_bytes(const P2PTraits& g, int block, int W) {
  return static_cast<size_t>(W) * (static_cast<size_t>(g.nwl) * 4 * block +
                                   (4 + static_cast<size_t>(g.cs_bytes)) * static_cast<size_t>(block / g.lanes));
}
bool ref_lds_cells(const P2PTraits& g, int W, int block) {
  return ref_lds_queue(g) && W <= 8 && ref_lds_bytes(g, true, block) + ref_lds_cell_bytes(g, block, W) <= 80 * 1024;
}
constexpr int kRefLdsCellsMinTicks = 24, kRefLdsQMinTicks = 4, kRefSpecBranches = 16;

// ---- kernels.hpp at bc5fca4
Ref ref_as_m(const P2PTraits& g, const P2PLaunchFacts& p, bool kSpec, bool kSparse, bool kNet, bool kMtf, bool kLog) {
  size_t lds = ref_lds_bytes(g, false, p.block);
  if ((!kSpec || g.inlane_fan) && !kNet && ref_lds_queue(g)) {
    const bool kHasQ = (!kSpec || (RB_SPEC_Q && g.inlane_fan)) && !kNet && g.lanes > 1;
    if (ref_lds_cells(g, p.W, p.block) && p.T >= kRefLdsCellsMinTicks && (!kSpec || !p.fan_generic) &&
        !(kHasQ && p.many_waves)) {
      const uint32_t k = (!p.sync_ticks && !kSpec) ? flags(kSpec, kSparse, kNet, true, !kSpec, false, kMtf, false, false, kLog)
                                                   : flags(kSpec, kSparse, kNet, true, false, false, kMtf, false, false, kLog);
      lds = ref_lds_bytes(g, true, p.block) + ref_lds_cell_bytes(g, p.block, p.W);
      return {k, lds, true};
    }
  }
  if ((!kSpec || (RB_SPEC_Q && g.inlane_fan)) && !kNet && ref_lds_queue(g) && g.lanes > 1) {
    if (p.T >= kRefLdsQMinTicks && (!kSpec || (p.many_waves && !p.fan_generic))) {
      const uint32_t k = flags(kSpec, kSparse, kNet, false, false, false, kMtf, true, false, kLog);
      lds = ref_lds_bytes(g, true, p.block);
      return {k, lds, true};
    }
  }
  if (!kSpec && !kNet) {
    if (p.T == 1) return {flags(kSpec, kSparse, kNet, false, false, false, kMtf, false, true, kLog), lds, false};
  }
  return {flags(kSpec, kSparse, kNet, false, false, false, kMtf, false, false, kLog), lds, false};
}
Ref ref_as_l(const P2PTraits& g, const P2PLaunchFacts& p, bool kSpec, bool kSparse, bool kNet, bool kLog) {
  if (kSpec) {
    if (g.alphabet > static_cast<uint32_t>(kRefSpecBranches)) return ref_as_m(g, p, kSpec, kSparse, kNet, true, kLog);
    else if (g.alphabet > static_cast<uint32_t>(p.fan_k)) return ref_as_m(g, p, kSpec, kSparse, kNet, true, kLog);
  }
  return ref_as_m(g, p, kSpec, kSparse, kNet, false, kLog);
}
Ref ref_as(const P2PTraits& g, const P2PLaunchFacts& p, bool kSpec, bool kSparse, bool kNet) {
  if (p.tick_log) return ref_as_l(g, p, kSpec, kSparse, kNet, true);
  return ref_as_l(g, p, kSpec, kSparse, kNet, false);
}
Ref ref_launch_p2p(const P2PTraits& g, const P2PLaunchFacts& p) {
  const bool kFanout = g.fanout;
  if (p.packets) {
    size_t lds = ref_lds_bytes(g, false, p.block);
    if (ref_lds_queue(g)) {
      if (ref_lds_cells(g, p.W, p.block) && p.T >= kRefLdsCellsMinTicks) {
        lds = ref_lds_bytes(g, true, p.block) + ref_lds_cell_bytes(g, p.block, p.W);
        return {flags(false, false, false, true, false, true), lds, true};
      }
    }
    if (p.T == 1) return {flags(false, false, false, false, false, true, false, false, true), lds, false};
    return {flags(false, false, false, false, false, true), lds, false};
  }
  if (p.ds_on || p.peer_on) {
    if (p.sparse) return ref_as(g, p, false, true, true);
    if (kFanout && p.spec_on && !p.peer_on) return ref_as(g, p, kFanout, false, true);
    return ref_as(g, p, false, false, true);
  }
  if (p.sparse) return ref_as(g, p, false, true, false);
  if (kFanout && p.spec_on) return ref_as(g, p, kFanout, false, false);
  return ref_as(g, p, false, false, false);
}

// ---- the games, from games.hpp: {lanes, players, input bytes, NWL, sizeof(CS), alphabet, fan-out, in-lane fan-out}
struct Game {
  const char* name;
  P2PTraits t;
};
const Game kGames[] = {
    {"ex_game P=2 (ExGame<2, true>)", {2, 2, 1, 5, 2, 16u, true, true}},
    {"ex_game P=4 (ExGame<4, true>)", {4, 4, 1, 5, 2, 16u, true, true}},
    {"brawler P=2 (Brawler<2>)", {64, 2, 1, 32, 2, 256u, true, false}},
    {"stub (StubGame)", {1, 2, 4, 1, 8, 0xFFFFFFFFu, false, false}},
};
}  // namespace

int main() {
  // the fits the trait sets are there for: ex_game's cells at W = 8, block 256 do, the brawler's do not
  if (!ref_lds_cells(kGames[0].t, 8, 256) || !ref_lds_cells(kGames[1].t, 8, 256) || ref_lds_cells(kGames[2].t, 8, 256)) {
    std::printf("FAIL: the LDS-cell fit of the trait sets is not the one intended\n");
    return 1;
  }
  const int Ts[] = {1, 2, 3, 4, 23, 24, 50}, Ws[] = {8, 9}, Ks[] = {8, 16};
  long cases = 0, bad = 0;
  for (const Game& g : kGames) {
    std::set<uint32_t> seen;
    for (int T : Ts)
      for (int W : Ws)
        for (int K : Ks)
          for (unsigned b = 0; b < (1u << 9); ++b) {  // the nine boolean facts
            const P2PLaunchFacts f{T, W, 256, (b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, K,
                                   (b & 16) != 0, (b & 32) != 0, (b & 64) != 0, (b & 128) != 0, (b & 256) != 0};
            const Ref r = ref_launch_p2p(g.t, f);
            const P2PChoice c = p2p_choose(g.t, f);
            ++cases;
            const bool attr = (c.variant & (kP2PLdsC | kP2PQ)) != 0;  // launch_p2p's hipFuncSetAttribute condition
            if (c.variant != r.v || c.lds != r.lds || attr != r.set_attr || !p2p_variant_valid(c.variant) ||
                !p2p_variant_reachable(g.t, c.variant)) {
              if (++bad <= 20)
                std::printf("MISMATCH %s T=%d W=%d K=%d facts=0x%x: was 0x%x lds %zu attr %d, is 0x%x lds %zu attr %d, "
                            "valid %d reachable %d\n", g.name, T, W, K, b, r.v, r.lds, r.set_attr, c.variant, c.lds, attr,
                            p2p_variant_valid(c.variant), p2p_variant_reachable(g.t, c.variant));
            }
            seen.insert(c.variant);
          }
    unsigned reachable = 0;
    for (uint32_t v = 0; v < kP2PVariants; ++v) reachable += p2p_variant_reachable(g.t, v) ? 1u : 0u;
    std::printf("%s: %zu distinct variants chosen, %u instantiated\n", g.name, seen.size(), reachable);
  }
  std::printf("%ld cases, %ld mismatches (RB_SPEC_Q=%d)\n", cases, bad, RB_SPEC_Q);
  return bad ? 1 : 0;
}
