// ggrs_amd/csrc/p2p_variant.hpp — which p2p_kernel instantiation (p2p.hpp) a P2P launch runs.  A variant
// is a set of P2PFlag bits, p2p_kernel's second template argument; p2p_choose is the whole rule, from the
// game (P2PTraits) and the launch (P2PLaunchFacts) to the variant and its dynamic LDS size.  Plain C++17,
// no device code: GameOpsT::launch_p2p (kernels.hpp) and the host tests (tests/check_p2p_variant.cpp) share it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "planner.hpp"  // kQueueLen

namespace rb {

// Spec / Sparse / Net: the fan-out select, sparse saving, the network-fed bookkeeping; LdsC: the snapshot
// and input rings in LDS; Async: lane-asynchronous ticks; Wire: packet-fed ticks; Mtf: the fan-out's
// candidates from move-to-front lists; Q: the input ring alone in LDS; One: the tick count compiled in
// as 1; Log: the launch writes the tick log.  (What each compiles in: p2p.hpp, above p2p_kernel.)
enum P2PFlag : uint32_t {
  kP2PSpec = 1u << 0, kP2PSparse = 1u << 1, kP2PNet = 1u << 2, kP2PLdsC = 1u << 3, kP2PAsync = 1u << 4,
  kP2PWire = 1u << 5, kP2PMtf = 1u << 6, kP2PQ = 1u << 7, kP2POne = 1u << 8, kP2PLog = 1u << 9,
  kP2PVariants = 1u << 10,  // the flag sets are 0 .. kP2PVariants - 1
};
// The flag sets p2p_kernel compiles for (its static assert).
constexpr bool p2p_variant_valid(uint32_t v) {
  const auto any = [v](uint32_t m) { return (v & m) != 0; };
  return v < kP2PVariants &&
         // lane-asynchronous ticks: plain or sparse path, LDS cells
         !(any(kP2PAsync) && (!any(kP2PLdsC) || any(kP2PSpec | kP2PNet))) &&
         // packet-fed ticks: the plain lock-step path; the tick log shares its parameter word with their pk_status
         !(any(kP2PWire) && any(kP2PSpec | kP2PSparse | kP2PNet | kP2PAsync | kP2PLog)) &&
         // one-tick launches keep the cells in HBM; desync detection reads HBM cells mid-launch
         !(any(kP2POne) && any(kP2PLdsC | kP2PAsync | kP2PQ)) && !(any(kP2PLdsC) && any(kP2PNet));
}

// Speculative fan-out: branch k holds candidate input cand[k] for one remote
// player over its unconfirmed frames.  Up to kSpecBranches
// candidates: the game's whole input alphabet when it has at most that many
// values (ex_game's 4 bits: cand[k] = k), else the K most likely values
// (fan_candidates in p2p.hpp).
constexpr int kSpecBranches = 16;

// What the rule reads of a game (p2p.hpp p2p_traits<G>()): kLanes, kPlayers, kInputBytes, NWL, sizeof(CS),
// InputAlphabet<G>, whether the two-launch fan-out exists (GameOpsT::kFanout), inlane_fan<G>().
struct P2PTraits {
  int lanes, players, input_bytes, nwl, cs_bytes;
  uint32_t alphabet;
  bool fanout, inlane_fan;
};

// LDS queues: 1-byte inputs, one player per lane (ex_game lane per player, the brawler).
constexpr bool p2p_lds_queue(const P2PTraits& t) { return t.input_bytes == 1 && (t.lanes > 1 || t.players == 1); }
// ... in a launch whose snapshot ring is (kLdsC) or is not in LDS.  Launches of
// few ticks keep the snapshot ring in HBM, and the input ring too: filling the
// LDS copy (byte loads in dependent rounds) and writing it back cost more than
// the handful of ring reads a short launch makes (measured, one tick per
// launch at 65,536 sessions: 14.8 -> 13.1 us, the packet-fed tick 18.9 -> 16.7).
#ifndef RB_SHORT_HBM_RING
#define RB_SHORT_HBM_RING 1  // 0: the LDS input ring in every launch (A/B builds)
#endif
constexpr bool p2p_lds_queue_in(const P2PTraits& t, bool ldsc) { return p2p_lds_queue(t) && (ldsc || !RB_SHORT_HBM_RING); }
constexpr size_t p2p_lds_bytes(const P2PTraits& t, bool ldsc, int block) {
  return p2p_lds_queue_in(t, ldsc) ? static_cast<size_t>(kQueueLen) * static_cast<size_t>(block) : 0;
}
// The snapshot ring in LDS (p2p_kernel kLdsC): for the launch, the W cells
// (words [W][NWL][block], frame tags and checksums [W][block / kLanes]) live
// after the queue in LDS; the launch loads them from HBM first and writes
// them back last.  Every SaveGameState and LoadGameState inside is an LDS
// access, and the tick loop issues no global store at all: CDNA's vmcnt
// retires loads and stores in issue order, so with a tick's snapshot stores
// in flight, waiting for the next tick's prefetched deliveries would wait for
// the stores too (the compiler cannot count stores issued in a loop of
// data-dependent length and drains the counter).  Up to kLdsCellsMaxW cells:
// at W = 8, 512 threads per CU (two waves per SIMD) take 156 KiB of the 160.
constexpr int kLdsCellsMaxW = 8;
constexpr size_t p2p_lds_cell_bytes(const P2PTraits& t, int block, int W) {
  return static_cast<size_t>(W) * (static_cast<size_t>(t.nwl) * 4 * block +
                                   (4 + static_cast<size_t>(t.cs_bytes)) * static_cast<size_t>(block / t.lanes));
}
// ... when the queue and the cells of a block fit half of a CU's 160 KiB (two
// blocks per CU): ex_game's 40 B cells do (79 KiB at 256 threads, W = 8), the
// brawler's 8 KiB cells do not and stay in HBM.
constexpr size_t kLdsPerBlockMax = 80 * 1024;
#ifndef RB_LDS_CELLS_MIN_TICKS
#define RB_LDS_CELLS_MIN_TICKS 24
#endif
// launches of fewer ticks keep the cells in HBM (and lock-step ticks): copying the
// ring in and out costs more than it saves below about 24 ticks (measured: HBM
// cells 4.8 us per tick at 16 ticks per launch, LDS cells 4.1 at 32)
constexpr int kLdsCellsMinTicks = RB_LDS_CELLS_MIN_TICKS;
// Launches of kLdsQMinTicks up to kLdsCellsMinTicks ticks keep the cells in HBM but the input ring
// in LDS (p2p_kernel kQ; plain path and sparse saving, ex_game's lane-per-player layout).  Measured
// at 65,536 sessions, us per tick (HBM ring / LDS ring / LDS cells): 2 ticks per launch 7.6 / 8.0 /
// 12.7, 4: 6.34 / 6.08 / 8.44, 8: 5.57 / 5.02 / 5.97, 16: 5.07 / 4.36 / 4.55 (round 4, interleaved A/B, tools/ab.py).
#ifndef RB_LDSQ_MIN_TICKS
#define RB_LDSQ_MIN_TICKS 4
#endif
constexpr int kLdsQMinTicks = RB_LDSQ_MIN_TICKS;
constexpr bool p2p_lds_cells(const P2PTraits& t, int W, int block) {
  return p2p_lds_queue(t) && W <= kLdsCellsMaxW &&
         p2p_lds_bytes(t, true, block) + p2p_lds_cell_bytes(t, block, W) <= kLdsPerBlockMax;
}
// RB_SPEC_Q: the in-kernel fan-out of a batch with more than two waves per SIMD keeps its cells in HBM
// and only the input ring in LDS (kQ), capped at RB_SPEC_Q_WAVES waves per SIMD, instead of the LDS
// snapshot ring's two workgroups per CU
#ifndef RB_SPEC_Q
#define RB_SPEC_Q 0
#endif

// Where a path (kSpec, kNet) of a game can keep its rings; the run-time half is in p2p_choose.
// kLdsC: with the fan-out only for the in-kernel one (fanout_kernel reads the HBM cells between ticks)
constexpr bool p2p_can_ldsc(const P2PTraits& t, bool spec, bool net) {
  return (!spec || t.inlane_fan) && !net && p2p_lds_queue(t);
}
constexpr bool p2p_can_q(const P2PTraits& t, bool spec, bool net) {
  return (!spec || (RB_SPEC_Q && t.inlane_fan)) && !net && p2p_lds_queue(t) && t.lanes > 1;
}
constexpr bool p2p_can_one(bool spec, bool net) { return !spec && !net; }

// A batch puts more than two waves on a SIMD of its device (P2PParams / RunParams many_waves).
constexpr bool many_waves_per_simd(int Spad, int lanes, int simds) {
  return static_cast<uint64_t>(Spad) * static_cast<uint64_t>(lanes) > 2ull * 64ull * static_cast<uint64_t>(simds);
}

// What the rule reads of P2PParams and the launch (packets, tick_log: non-null; ds_on: ds.interval > 0).
struct P2PLaunchFacts {
  int T, W, block;
  bool packets, sparse, spec_on, fan_generic;
  int fan_k;
  bool sync_ticks, many_waves, tick_log, ds_on, peer_on;
};
struct P2PChoice {
  uint32_t variant;  // P2PFlag set
  size_t lds;        // dynamic LDS bytes of the launch
};

inline P2PChoice p2p_choose(const P2PTraits& t, const P2PLaunchFacts& f) {
  // the snapshot ring in LDS (p2p_lds_cell_bytes) for launches of many ticks: it is copied in and
  // written back whole, which short launches (the wire path's one tick per launch) do not repay
  const bool cells_pay = p2p_lds_cells(t, f.W, f.block) && f.T >= kLdsCellsMinTicks;
  const size_t lds_cells = p2p_lds_bytes(t, true, f.block) + p2p_lds_cell_bytes(t, f.block, f.W);
  const size_t lds_hbm = p2p_lds_bytes(t, false, f.block);  // (the HBM-cell launches)
  if (f.packets) {  // packet-fed ticks (rb_p2p_run_ticks_packets: the plain path, lock-step ticks)
    if (cells_pay) return {kP2PWire | kP2PLdsC, lds_cells};
    if (f.T == 1) return {kP2PWire | kP2POne, lds_hbm};  // one tick per launch (kOne, below)
    return {kP2PWire, lds_hbm};
  }
  // ---- the path
  const bool net = f.ds_on || f.peer_on;  // desync detection / peers' connect-status reports on
  // sparse saving and the fan-out exclude each other (rb_p2p_create); the fan-out assumes connected
  // queues (peer_on: the peers' reports can disconnect one)
  const bool spec = !f.sparse && t.fanout && f.spec_on && !f.peer_on;
  // the fan-out's candidates: the alphabet itself when it has at most K values, else the queues'
  // move-to-front lists (kMtf); ex_game (16 inputs) builds both, larger alphabets only the lists
  const bool mtf = spec && (t.alphabet > static_cast<uint32_t>(kSpecBranches) || t.alphabet > static_cast<uint32_t>(f.fan_k));
  // time sync on (P2PParams::tick_log; never a packet-fed launch): the instantiations that write the tick log
  uint32_t v = (net ? kP2PNet : 0u) | (f.sparse ? kP2PSparse : 0u) | (spec ? kP2PSpec : 0u) | (mtf ? kP2PMtf : 0u) |
               (f.tick_log ? kP2PLog : 0u);
  // ---- the storage
  // the LDS cells ... unless the batch puts more than two waves on a SIMD and the plain or sparse
  // path can keep only the input ring in LDS (kQ below): the LDS cells (79 KiB per 256 threads) fit
  // two workgroups per CU, kQ four (131,072 sessions, lag 1-4: 6.72 -> 5.25 us per tick; at 65,536
  // sessions, two waves per SIMD, the LDS cells stay faster, 3.43 against 3.81)
  const bool q_for_many = p2p_can_q(t, spec, net) && f.many_waves;
  if (p2p_can_ldsc(t, spec, net) && cells_pay && (!spec || !f.fan_generic) && !q_for_many) {
    // lane-asynchronous ticks (plain path and sparse saving) unless the batch asked for lock-step
    // ticks; the fan-out runs lock-step ticks
    const bool async = !f.sync_ticks && !spec;
    return {v | kP2PLdsC | (async ? kP2PAsync : 0u), lds_cells};
  }
  // the input ring alone in LDS
  if (p2p_can_q(t, spec, net) && f.T >= kLdsQMinTicks && (!spec || (f.many_waves && !f.fan_generic)))
    return {v | kP2PQ, p2p_lds_bytes(t, true, f.block)};
  // live play, one tick per launch: the tick count compiled in (p2p_kernel kOne: 121 -> 99 VGPRs, no
  // SGPR spills; 9.70 -> 9.59 us at 65,536 sessions, packet-fed 11.07 -> 10.45; r06_ab_one_tick.log)
  if (p2p_can_one(spec, net) && f.T == 1) v |= kP2POne;
  return {v, lds_hbm};
}

// The variants GameOpsT instantiates for a game: those p2p_choose can return for it, whatever the launch.
constexpr bool p2p_variant_reachable(const P2PTraits& t, uint32_t v) {
  const auto has = [v](uint32_t m) { return (v & m) != 0; };
  const bool spec = has(kP2PSpec), net = has(kP2PNet);
  if (!p2p_variant_valid(v)) return false;
  if (has(kP2PWire)) return !has(kP2PMtf | kP2PQ) && (!has(kP2PLdsC) || p2p_lds_queue(t));
  if (spec && (!t.fanout || has(kP2PSparse))) return false;
  // (the fan-out without kMtf is also built for alphabets above kSpecBranches, which never run it: the
  // brawler's four such kernels have been in the library since kMtf and stay until a change of their own)
  if (has(kP2PMtf) && !spec) return false;
  if (has(kP2PLdsC) && !p2p_can_ldsc(t, spec, net)) return false;
  if (has(kP2PQ) && (has(kP2PLdsC) || !p2p_can_q(t, spec, net))) return false;
  if (has(kP2POne) && !p2p_can_one(spec, net)) return false;
  return true;
}

}  // namespace rb
