// tests/check_protocol.cpp — drives ggrs_amd/csrc/protocol_step.hpp, the per-endpoint step of
// rb_endpoint_protocol_poll_all, on the host (tests/test_protocol.py writes the schedule and compares
// the output with its model).  A stand-alone program: build it with -fsanitize=address,undefined to
// have every read of a datagram checked against a heap buffer of exactly its bytes.
//
//   check_protocol run FILE      the schedule of FILE, one output line per endpoint and call
//   check_protocol corrupt SEED N   N steps over state rows and inputs of random bytes
//
// FILE: "P E M sync_slots stride calls", then per call "now loads", `loads` lines
// "e state remaining n0..n7 valid next stamp0..stamp4 sent last_newest remote_magic" (state rows the
// caller writes before the call), and E lines "magic start disconnected ack_owed reply_owed received
// newest acked length reports | M x (length hex|-) | M x nonce".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "protocol_step.hpp"

using namespace rb;

static void print(int c, int e, const PrState& t, const PrOutput& o, int sync_slots) {
  std::printf("%d %d %u %d", c, e, t.state, t.sync_remaining);
  for (int i = 0; i < kPrNonces; ++i) std::printf(" %u", t.nonces[i]);
  std::printf(" %u %u %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %u |", t.valid, t.next, t.last_send,
              t.last_input_recv, t.last_quality_report, t.shutdown_at, t.stats_start, t.packets_sent, t.last_newest,
              t.remote_magic);
  std::printf(" %d %u %u %u %u %d %u %d %u %d %u %u |", o.input_length, o.ack_due, o.reply_due, o.report_due, o.keepalive_due,
              o.sync_msgs, o.events, o.sync_count, o.liveness_received, o.send_queue_len, o.synchronized, o.status);
  for (int m = 0; m < sync_slots; ++m) {
    if (m >= o.sync_msgs) {
      std::printf(" -");
      continue;
    }
    unsigned char b[12];
    std::memcpy(b, o.msg[m], 12);
    std::printf(" ");
    for (int i = 0; i < kPrSyncBytes; ++i) std::printf("%02x", b[i]);
  }
  std::printf("\n");
}

// the slot's digest from a heap buffer of exactly min(length, stride) bytes
static void digest(const std::string& hex, int32_t length, int64_t stride, uint32_t& tag, uint32_t& x) {
  const int32_t avail = length < stride ? length : static_cast<int32_t>(stride);
  const size_t n = avail > 0 ? static_cast<size_t>(avail) : 0;
  unsigned char* buf = static_cast<unsigned char*>(std::malloc(n ? n : 1));
  for (size_t i = 0; i < n; ++i) buf[i] = static_cast<unsigned char>(std::stoi(hex.substr(2 * i, 2), nullptr, 16));
  uint32_t w[3] = {0u, 0u, 0u};
  std::memcpy(w, buf, n < 12 ? n : 12);
  std::free(buf);
  pr_digest(avail, w[0], w[1], w[2], tag, x);
}

static int run(const char* path) {
  std::ifstream f(path);
  int P, E, M, sync_slots, calls;
  int64_t stride;
  if (!(f >> P >> E >> M >> sync_slots >> stride >> calls)) return 2;
  std::vector<PrState> st(static_cast<size_t>(E), PrState{});
  for (int c = 0; c < calls; ++c) {
    int64_t now;
    int loads;
    if (!(f >> now >> loads)) return 2;
    for (int l = 0; l < loads; ++l) {
      int e;
      f >> e;
      PrState& t = st[static_cast<size_t>(e)];
      f >> t.state >> t.sync_remaining;
      for (int i = 0; i < kPrNonces; ++i) f >> t.nonces[i];
      f >> t.valid >> t.next >> t.last_send >> t.last_input_recv >> t.last_quality_report >> t.shutdown_at >> t.stats_start >>
          t.packets_sent >> t.last_newest >> t.remote_magic;
    }
    for (int e = 0; e < E; ++e) {
      PrInput in{};
      in.now = now;
      in.slots = M;
      in.sync_slots = sync_slots;
      std::string bar;
      f >> in.local_magic >> in.start >> in.disconnected >> in.ack_owed >> in.reply_owed >> in.received >> in.newest >> in.acked >>
          in.length >> in.reports >> bar;
      for (int m = 0; m < M; ++m) {
        int32_t length;
        std::string hex;
        f >> length >> hex;
        digest(hex == "-" ? std::string() : hex, hex == "-" ? 0 : length, stride, in.tag[m], in.x[m]);
      }
      f >> bar;
      for (int m = 0; m < M; ++m) f >> in.nonces[m];
      if (!f) return 2;
      PrState t = st[static_cast<size_t>(e)];
      PrOutput o;
      if (pr_step(t, in, o)) st[static_cast<size_t>(e)] = t;
      print(c, e, st[static_cast<size_t>(e)], o, sync_slots);
    }
  }
  return 0;
}

// State rows and inputs of random bytes: nothing the step does may depend on their being sound.
static int corrupt(uint64_t seed, int n) {
  std::mt19937_64 rng(seed);
  uint64_t folded = 0;
  for (int k = 0; k < n; ++k) {
    PrState t;
    PrInput in;
    uint64_t* a = reinterpret_cast<uint64_t*>(&t);
    for (size_t i = 0; i < sizeof(t) / 8; ++i) a[i] = rng();
    uint64_t* b = reinterpret_cast<uint64_t*>(&in);
    for (size_t i = 0; i < sizeof(in) / 8; ++i) b[i] = rng();
    static_assert(sizeof(PrState) % 8 == 0 && sizeof(PrInput) % 8 == 0, "filled in words");
    // what the entry point validates, and what the kernel computes itself, stays in range
    in.slots = 1 + static_cast<int32_t>(rng() % kPrMaxSlots);
    in.sync_slots = 1 + static_cast<int32_t>(rng() % kPrMaxSlots);
    in.reports = static_cast<int32_t>(rng() % 9);
    if (k % 3 == 0) t.state = static_cast<uint32_t>(rng() % 6);  // known states too, with the rest corrupt
    if (k % 5 == 0) in.now = static_cast<int64_t>(rng() >> 1);
    for (int m = 0; m < kPrMaxSlots; ++m) {
      unsigned char raw[16];
      for (auto& r : raw) r = static_cast<unsigned char>(rng());
      if (m % 2) raw[2] = static_cast<unsigned char>(rng() % 2), raw[3] = raw[4] = raw[5] = 0;  // a sync kind
      const int32_t avail = static_cast<int32_t>(rng() % 17);
      std::string hex;
      char two[3];
      for (int i = 0; i < avail; ++i) std::snprintf(two, 3, "%02x", raw[i]), hex += two;
      digest(hex, avail, 16, in.tag[m], in.x[m]);
    }
    PrOutput o;
    pr_step(t, in, o);
    if (o.sync_msgs < 0 || o.sync_msgs > in.sync_slots || o.synchronized > 1u || o.liveness_received > 1u) return 1;
    folded = folded * 1099511628211ull + t.state + o.sync_msgs + static_cast<uint64_t>(t.packets_sent);
  }
  std::printf("corrupt ok %d %" PRIu64 "\n", n, folded);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "run") == 0) return run(argv[2]);
  if (argc == 4 && std::strcmp(argv[1], "corrupt") == 0) return corrupt(std::strtoull(argv[2], nullptr, 10), std::atoi(argv[3]));
  std::fprintf(stderr, "usage: check_protocol run FILE | corrupt SEED N\n");
  return 2;
}
