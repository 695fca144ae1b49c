// tests/check_session_record.cpp — the session record's layout (ggrs_amd/csrc/session_record.hpp
// record_layout) over synthetic plane lists shaped like the engines' (p2p_engine.hip *_planes,
// spectator_engine.hip spectator_planes): ex_game P = 2 and P = 4, a brawler-sized state, with and
// without the desync, peer, time-sync and pace groups.  Every plane's bytes lie inside the record
// behind the header, no two overlap, each part is aligned to its element size, record_bytes is a
// multiple of 16, and the fingerprint changes when any one plane's shape or any configuration
// word changes.  No GPU: tests/test_migrate.py compiles and runs this.
#include <algorithm>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "session_record.hpp"

using namespace rb;

namespace {
int g_fail = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++g_fail;                     \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");            \
    }                               \
  } while (0)

// the state planes of PlaneSet::state: groups of four words, then a pair, then a single word
void state(std::vector<PlaneShape>& p, uint32_t nw, uint32_t lanes, uint32_t cells) {
  const uint32_t q4 = nw / 4, r = nw % 4;
  if (q4) p.push_back({16, q4, cells, lanes});
  if (r >= 2) p.push_back({8, 1, cells, lanes});
  if (r & 1) p.push_back({4, 1, cells, lanes});
}

struct Shape {
  const char* name;
  uint32_t nw, lanes, cs_bytes, input_bytes, P, W;
};

std::vector<PlaneShape> planes(const Shape& s, bool desync, bool peer, bool ts, bool pace) {
  std::vector<PlaneShape> p;
  state(p, s.nw, s.lanes, 1);    // live
  state(p, s.nw, s.lanes, s.W);  // snapshots
  p.push_back({s.cs_bytes, s.W, 1, 1});
  p.push_back({4, s.W, 1, 1});                // tags
  p.push_back({s.input_bytes, 128 * s.P, 1, 1});  // the input ring
  p.push_back({4, 1, 1, 1});                  // status
  p.push_back({4, 1, 1, 1});                  // trace
  p.push_back({4, 61, 1, 1});                 // bookkeeping rows
  if (desync) {
    p.push_back({4, 32, 1, 1});
    p.push_back({8, 32, 1, 1});
    p.push_back({4, 128, 1, 1});
    p.push_back({4, 3, 4, 1});
    p.push_back({4, 1, 1, 1});
    p.push_back({4, 1, 1, 1});
    p.push_back({4, 8, 1, 1});
    p.push_back({4, 8, 1, 1});
    p.push_back({8, 128, 1, 1});  // carry-only from here
    p.push_back({8, 128, 1, 1});
    p.push_back({4, 16, 1, 1});
    p.push_back({8, 16, 1, 1});
    p.push_back({8, 8, 1, 1});
    p.push_back({8, 8, 1, 1});
  }
  if (peer) {
    p.push_back({4, 16, 1, 1});
    p.push_back({4, 16, 1, 1});
  }
  p.push_back({4, 2, 1, 1});  // export rows
  if (ts) {
    p.push_back({4, 40, 1, 1});
    p.push_back({4, 2 * 40 * 4, 1, 1});
  }
  if (pace)
    for (int i = 0; i < 3; ++i) p.push_back({4, 1, 1, 1});
  return p;
}

int check(const char* what, const std::vector<PlaneShape>& p, const std::vector<uint32_t>& cfg) {
  const RecordLayout lay = record_layout(p, cfg);
  CHECK(lay.off.size() == p.size(), "%s: %zu offsets for %zu planes", what, lay.off.size(), p.size());
  CHECK(lay.record_bytes % 16 == 0, "%s: record_bytes %zu is not a multiple of 16", what, lay.record_bytes);
  std::vector<std::pair<size_t, size_t>> spans;  // [begin, end)
  spans.push_back({0, kRecordHeaderBytes});
  size_t payload = 0;
  for (size_t i = 0; i < p.size(); ++i) {
    const size_t bytes = plane_part_bytes(p[i]);
    CHECK(lay.off[i] % p[i].esize == 0, "%s: plane %zu at %zu is not aligned to %u", what, i, lay.off[i], p[i].esize);
    CHECK(lay.off[i] >= kRecordHeaderBytes && lay.off[i] + bytes <= lay.record_bytes, "%s: plane %zu [%zu, %zu) outside the record of %zu",
          what, i, lay.off[i], lay.off[i] + bytes, lay.record_bytes);
    spans.push_back({lay.off[i], lay.off[i] + bytes});
    payload += bytes;
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    CHECK(spans[i - 1].second <= spans[i].first, "%s: parts [%zu, %zu) and [%zu, %zu) overlap", what, spans[i - 1].first,
          spans[i - 1].second, spans[i].first, spans[i].second);
  // padding is alignment only: less than 16 bytes per plane and at the end
  CHECK(lay.record_bytes <= kRecordHeaderBytes + payload + 16 * (p.size() + 1), "%s: %zu bytes for a payload of %zu", what,
        lay.record_bytes, payload);
  // the fingerprint: any one field of any one plane, the plane count, the order, any configuration word
  std::set<uint64_t> seen{lay.fingerprint};
  int variants = 0;
  auto differs = [&](const std::vector<PlaneShape>& q, const std::vector<uint32_t>& c, const char* change, size_t i) {
    const uint64_t f = record_layout(q, c).fingerprint;
    CHECK(f != lay.fingerprint, "%s: the fingerprint survives %s of entry %zu", what, change, i);
    seen.insert(f);
    ++variants;
  };
  for (size_t i = 0; i < p.size(); ++i) {
    std::vector<PlaneShape> q = p;
    q[i].esize *= 2;
    differs(q, cfg, "another element size", i);
    q = p;
    q[i].rows_in += 1;
    differs(q, cfg, "another row", i);
    q = p;
    q[i].groups += 1;
    differs(q, cfg, "another group", i);
    q = p;
    q[i].cps += 1;
    differs(q, cfg, "another lane", i);
    q = p;
    std::swap(q[i].rows_in, q[i].groups);
    if (p[i].rows_in != p[i].groups) differs(q, cfg, "rows and groups swapped", i);
    q = p;
    q.erase(q.begin() + static_cast<long>(i));
    differs(q, cfg, "a missing plane", i);
  }
  for (size_t i = 0; i < cfg.size(); ++i) {
    std::vector<uint32_t> c = cfg;
    c[i] ^= 1u;
    differs(p, c, "another configuration word", i);
  }
  CHECK(record_layout(p, cfg).fingerprint == lay.fingerprint && record_layout(p, cfg).record_bytes == lay.record_bytes,
        "%s: the layout is not a function of its arguments", what);
  return variants;
}
}  // namespace

int main() {
  const Shape shapes[] = {{"ex_game P=2", 7, 2, 16, 1, 2, 8},
                          {"ex_game P=4", 7, 4, 16, 1, 4, 8},
                          {"stub", 2, 1, 8, 4, 2, 9},
                          {"brawler", 32, 64, 16, 1, 2, 8}};
  int lists = 0, variants = 0;
  std::set<uint64_t> prints;
  for (const Shape& s : shapes)
    for (int m = 0; m < 16; ++m) {
      const bool desync = m & 1, peer = m & 2, ts = m & 4, pace = m & 8;
      const std::vector<uint32_t> cfg = {1u, 0u, s.P, s.W, s.input_bytes, s.nw, s.lanes, s.cs_bytes, 0u, 1u, 1u, 1u, 0u,
                                         desync ? 10u : 0u, peer ? 1u : 0u, ts ? 1u : 0u, ts ? 60u : 0u, 0u, 0u};
      char what[96];
      std::snprintf(what, sizeof what, "%s desync=%d peer=%d ts=%d pace=%d", s.name, desync, peer, ts, pace);
      variants += check(what, planes(s, desync, peer, ts, pace), cfg);
      prints.insert(record_layout(planes(s, desync, peer, ts, pace), cfg).fingerprint);
      ++lists;
    }
  CHECK(prints.size() == static_cast<size_t>(lists), "%zu fingerprints for %d plane lists", prints.size(), lists);
  // the brawler's record at W = 8: 9 cells of 32 words x 64 lanes, and the rest
  const RecordLayout b = record_layout(planes(shapes[3], false, false, false, false), {});
  CHECK(b.record_bytes > 9u * 32 * 64 * 4 && b.record_bytes < 9u * 32 * 64 * 4 + 4096, "brawler record of %zu bytes", b.record_bytes);
  std::printf("%d plane lists, %d variants, %d failures\n", lists, variants, g_fail);
  return g_fail ? 1 : 0;
}
