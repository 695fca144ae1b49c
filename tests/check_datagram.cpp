// tests/check_datagram.cpp — the per-endpoint datagram steps (ggrs_amd/csrc/datagram_step.hpp, the
// functions datagram.hip's kernels call) driven on the host over a schedule read from a file.
// Every datagram and every packet lives in a heap buffer of exactly its bytes and is read through
// bounded loaders, so a sanitizer build of this program sees any byte the steps read past a
// length.  No GPU.
//
//   check_datagram parse FILE
//     P E M stride packet_stride N            (E endpoints, M slots, N calls)
//     E remote magics
//     then N calls:  now_ms take              (take: the caller zeroes report_counts first)
//       then E * M datagrams, endpoint-major:  length hex|-   (hex: min(length, stride) bytes)
//     in/out words start at acked -1, frame_advantage 0, rtt_ms 0, report_counts 0 and carry over.
//     Prints per call and endpoint
//       call e received requested acked advantage rtt owed ping_lo ping_hi status length start count
//       | last[P] disconnected[P] | packet hex|- | count x (lo hi frame)
//
//   check_datagram build FILE
//     P M stride packet_stride N
//     then N endpoints:  magic now_ms input_len start ack requested  last[P] disconnected[P]
//                        ack_owed reply_owed ping_lo ping_hi report_due advantage keepalive
//                        K x (lo hi frame)  packet hex|-
//     Prints per endpoint  case count status  then count x ( length hex ).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "datagram_step.hpp"

using namespace rb;

namespace {

struct Bytes {  // a heap buffer of exactly n bytes
  std::unique_ptr<uint8_t[]> p;
  int64_t n = 0;
};

Bytes from_hex(const char* hex) {
  Bytes b;
  if (hex[0] == '-') return b;
  b.n = static_cast<int64_t>(std::strlen(hex) / 2);
  b.p.reset(new uint8_t[static_cast<size_t>(b.n)]);
  for (int64_t i = 0; i < b.n; ++i) {
    unsigned v = 0;
    std::sscanf(hex + 2 * i, "%2x", &v);
    b.p[static_cast<size_t>(i)] = static_cast<uint8_t>(v);
  }
  return b;
}

void print_hex(const uint8_t* d, int64_t n) {
  if (n <= 0) std::printf("-");
  for (int64_t i = 0; i < n; ++i) std::printf("%02x", d[i]);
}

DgChunk load_bounded(const Bytes& b, int32_t c) {  // chunk c of a buffer that ends where its bytes end
  DgChunk x{{0u, 0u, 0u, 0u}};
  const int64_t at = 16 * static_cast<int64_t>(c);
  if (at < b.n) std::memcpy(x.w, b.p.get() + at, static_cast<size_t>(b.n - at < 16 ? b.n - at : 16));
  return x;
}

bool read_token(std::FILE* f, std::string& out) {
  std::vector<char> buf(1 << 16);
  if (std::fscanf(f, "%65535s", buf.data()) != 1) return false;
  out = buf.data();
  return true;
}

struct Kept {  // an endpoint's state across parse calls
  int32_t acked = -1, advantage = 0, rtt = 0, count = 0;
  DgReport reports[kDgReportsKept];
};

template <int P>
int run_parse(std::FILE* f, int E, int M, int64_t stride, int64_t packet_stride, int N) {
  using Y = DgLayout<P>;
  constexpr int HW = Y::kHeadWords;
  std::vector<uint32_t> magic(static_cast<size_t>(E));
  for (auto& m : magic)
    if (std::fscanf(f, "%u", &m) != 1) return 2;
  std::vector<Kept> kept(static_cast<size_t>(E));
  for (int call = 0; call < N; ++call) {
    int64_t now = 0;
    int take = 0;
    if (std::fscanf(f, "%" SCNd64 " %d", &now, &take) != 2) return 2;
    for (int e = 0; e < E; ++e) {
      Kept& k = kept[static_cast<size_t>(e)];
      if (take) k.count = 0;
      std::vector<Bytes> dg(static_cast<size_t>(M));
      std::vector<int32_t> len(static_cast<size_t>(M));
      DgEndpoint ep = dg_endpoint(k.acked, k.advantage, k.rtt);
      std::vector<DgReport> fresh;
      for (int m = 0; m < M; ++m) {
        std::string hex;
        if (std::fscanf(f, "%d", &len[static_cast<size_t>(m)]) != 1 || !read_token(f, hex)) return 2;
        dg[static_cast<size_t>(m)] = from_hex(hex.c_str());
        const int32_t n = len[static_cast<size_t>(m)];
        if (n <= 0) continue;
        const int32_t avail = n < stride ? n : static_cast<int32_t>(stride);
        const Bytes& b = dg[static_cast<size_t>(m)];
        if (b.n != avail) return 3;  // the schedule's own mistake
        uint32_t w[HW] = {};
        std::memcpy(w, b.p.get(), static_cast<size_t>(avail < 4 * HW ? avail : 4 * HW));
        const uint32_t before = ep.report_slots;
        dg_parse_one<P>(w, avail, m, magic[static_cast<size_t>(e)], now, ep);
        if (ep.report_slots != before) fresh.push_back(dg_report_of<HW>(w));
      }
      const DgReportPlan plan = dg_report_plan(k.count, dg_popcount8(ep.report_slots));
      if (plan.drop > 0) ep.status |= kDgReportsDropped;
      std::vector<DgReport> all(k.reports, k.reports + plan.kept);
      all.insert(all.end(), fresh.begin(), fresh.end());
      for (int j = 0; j < plan.count; ++j) k.reports[j] = all[static_cast<size_t>(j + plan.drop)];
      k.count = plan.count;
      k.acked = ep.acked;
      k.advantage = ep.frame_advantage;
      k.rtt = ep.rtt_ms;
      std::printf("%d %d %u %u %d %d %d %u %" PRIu64 " %" PRIu64 " %u %d %d %d |", call, e, ep.received,
                  ep.disconnect_requested, ep.acked, ep.frame_advantage, ep.rtt_ms, ep.reply_owed, ep.ping_lo, ep.ping_hi,
                  ep.status, ep.input_slot >= 0 ? ep.payload_len : 0, ep.input_slot >= 0 ? ep.start_frame : 0, plan.count);
      for (int i = 0; i < P; ++i) std::printf(" %d", ep.peer_last[i]);
      for (int i = 0; i < P; ++i) std::printf(" %u", (ep.peer_disconnected >> i) & 1u);
      std::printf(" | ");
      if (ep.input_slot >= 0 && ep.payload_len > 0) {
        const Bytes& b = dg[static_cast<size_t>(ep.input_slot)];
        const int32_t n = ep.payload_len < packet_stride ? ep.payload_len : static_cast<int32_t>(packet_stride);
        Bytes row;  // whole 16-byte chunks, as the kernel's row
        row.n = (static_cast<int64_t>(n) + 15) / 16 * 16;
        row.p.reset(new uint8_t[static_cast<size_t>(row.n)]);
        dg_copy_from<Y::kPayload>([&](int32_t c) { return load_bounded(b, c); }, (Y::kPayload + ep.payload_len + 15) >> 4, n,
                                  [&](int32_t c, const DgChunk& x) { std::memcpy(row.p.get() + 16 * c, x.w, 16); });
        print_hex(row.p.get(), n);
      } else {
        std::printf("-");
      }
      std::printf(" |");
      for (int j = 0; j < plan.count; ++j)
        std::printf(" %" PRIu64 " %" PRIu64 " %d", k.reports[j].lo, k.reports[j].hi, k.reports[j].frame);
      std::printf("\n");
    }
  }
  return 0;
}

template <int P>
int run_build(std::FILE* f, int M, int64_t stride, int64_t packet_stride, int N) {
  for (int n = 0; n < N; ++n) {
    DgOwed o{};
    if (std::fscanf(f, "%u %" SCNd64 " %d %d %d %u", &o.magic, &o.now_ms, &o.input_len, &o.start_frame, &o.ack_frame,
                    &o.disconnect_requested) != 6)
      return 2;
    for (int i = 0; i < P; ++i)
      if (std::fscanf(f, "%d", &o.status_last[i]) != 1) return 2;
    for (int i = 0; i < P; ++i) {
      unsigned d = 0;
      if (std::fscanf(f, "%u", &d) != 1) return 2;
      o.status_disconnected |= (d ? 1u : 0u) << i;
    }
    if (std::fscanf(f, "%u %u %" SCNu64 " %" SCNu64 " %u %d %u", &o.ack_owed, &o.reply_owed, &o.ping_lo, &o.ping_hi,
                    &o.report_due, &o.frame_advantage, &o.keepalive_due) != 7)
      return 2;
    for (int k = 0; k < kDgReportsKept; ++k)
      if (std::fscanf(f, "%" SCNu64 " %" SCNu64 " %d", &o.reports[k].lo, &o.reports[k].hi, &o.reports[k].frame) != 3) return 2;
    std::string hex;
    if (!read_token(f, hex)) return 2;
    const Bytes pk = from_hex(hex.c_str());
    uint32_t status = 0;
    if (o.input_len > packet_stride) {
      status |= kDgMalformed;
      o.input_len = 0;
    }
    if (o.input_len > 0 && pk.n != o.input_len) return 3;
    std::vector<Bytes> rows;
    std::vector<int32_t> lens;
    auto fresh_row = [&]() -> uint8_t* {
      Bytes r;
      r.n = stride;
      r.p.reset(new uint8_t[static_cast<size_t>(stride)]);
      std::memset(r.p.get(), 0xEE, static_cast<size_t>(stride));
      rows.push_back(std::move(r));
      return rows.back().p.get();
    };
    const int32_t count = dg_build_endpoint<P>(
        o, M, stride, status,
        [&](int32_t, int32_t bytes) {
          uint8_t* out = fresh_row();
          lens.push_back(bytes);
          dg_emit_input<P>(o, [&](int32_t c) { return load_bounded(pk, c); },
                           [&](int32_t c, const DgChunk& x) { std::memcpy(out + 16 * c, x.w, 16); });
        },
        [&](int32_t, const DgFixed& m) {
          uint8_t* out = fresh_row();
          lens.push_back(m.len);
          std::memcpy(out, m.w, 32);
        });
    std::printf("%d %d %u", n, count, status);
    for (int32_t k = 0; k < count; ++k) {
      std::printf(" %d ", lens[static_cast<size_t>(k)]);
      print_hex(rows[static_cast<size_t>(k)].p.get(), lens[static_cast<size_t>(k)]);
    }
    std::printf("\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: check_datagram parse|build SCHEDULE\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[2], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  int rc = 2, P = 0, E = 0, M = 0, N = 0;
  int64_t stride = 0, packet_stride = 0;
  const bool parse = std::strcmp(argv[1], "parse") == 0;
  const bool header = parse ? std::fscanf(f, "%d %d %d %" SCNd64 " %" SCNd64 " %d", &P, &E, &M, &stride, &packet_stride, &N) == 6
                            : std::fscanf(f, "%d %d %" SCNd64 " %" SCNd64 " %d", &P, &M, &stride, &packet_stride, &N) == 5;
  if (header && M >= 1 && M <= kDgMaxSlots && stride >= 64 && stride % 16 == 0 && packet_stride >= 32 && packet_stride % 16 == 0) {
    if (parse) {
      rc = P == 1 ? run_parse<1>(f, E, M, stride, packet_stride, N) : P == 2 ? run_parse<2>(f, E, M, stride, packet_stride, N)
           : P == 3 ? run_parse<3>(f, E, M, stride, packet_stride, N) : P == 4 ? run_parse<4>(f, E, M, stride, packet_stride, N) : 2;
    } else {
      rc = P == 1 ? run_build<1>(f, M, stride, packet_stride, N) : P == 2 ? run_build<2>(f, M, stride, packet_stride, N)
           : P == 3 ? run_build<3>(f, M, stride, packet_stride, N) : P == 4 ? run_build<4>(f, M, stride, packet_stride, N) : 2;
    }
  }
  std::fclose(f);
  if (rc != 0) std::fprintf(stderr, "bad schedule (%d)\n", rc);
  return rc;
}
