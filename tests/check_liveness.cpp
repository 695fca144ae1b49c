// tests/check_liveness.cpp — the per-endpoint liveness step (ggrs_amd/csrc/liveness_step.hpp
// liveness_step, the function p2p_liveness_kernel calls) driven on the host over a schedule read
// from a file:
//   E N notify_start_ms disconnect_timeout_ms
//   then N polls, each a line:  now_ms  r[0] q[0]  r[1] q[1] ... r[E-1] q[E-1]
// (r: received, q: disconnect_requested, per endpoint).  Every endpoint starts unstamped with no
// flag; once a poll raised Disconnected for it, it stamps and raises nothing more (its endpoint no
// longer runs), as in the kernel.  Prints one line per poll and endpoint,
//   poll endpoint stamp flags kind:value ...
// which tests/test_liveness.py compares with its model.  No GPU.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "liveness_step.hpp"

using namespace rb;

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: check_liveness SCHEDULE\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int E = 0, N = 0, notify = 0, timeout = 0;
  if (std::fscanf(f, "%d %d %d %d", &E, &N, &notify, &timeout) != 4 || E <= 0 || N < 0) {
    std::fprintf(stderr, "bad header\n");
    std::fclose(f);
    return 2;
  }
  std::vector<int64_t> stamp(static_cast<size_t>(E), kLvUnstamped);
  std::vector<uint32_t> flags(static_cast<size_t>(E), 0u);
  std::vector<char> gone(static_cast<size_t>(E), 0);
  for (int k = 0; k < N; ++k) {
    int64_t now = 0;
    if (std::fscanf(f, "%" SCNd64, &now) != 1) {
      std::fprintf(stderr, "poll %d: missing clock\n", k);
      std::fclose(f);
      return 2;
    }
    for (int e = 0; e < E; ++e) {
      int r = 0, q = 0;
      if (std::fscanf(f, "%d %d", &r, &q) != 2) {
        std::fprintf(stderr, "poll %d: missing endpoint %d\n", k, e);
        std::fclose(f);
        return 2;
      }
      const size_t i = static_cast<size_t>(e);
      const LivenessStep s = liveness_step(stamp[i], flags[i], r != 0, q != 0, now, notify, timeout);
      stamp[i] = s.stamp;
      std::printf("%d %d %" PRId64, k, e, s.stamp);
      if (gone[i]) {
        std::printf(" %u\n", flags[i]);
        continue;
      }
      flags[i] = s.flags;
      std::printf(" %u", s.flags);
      for (int slot = 0; slot < kLvSlots; ++slot) {
        if (!((s.events >> slot) & 1u)) continue;
        const int32_t kind = liveness_event_kind(slot);
        std::printf(" %d:%d", kind, kind == kLvInterrupted ? s.value : 0);
        if (kind == kLvDisconnected) gone[i] = 1;
      }
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
