// tests/check_wire_group.cpp — drives ggrs_amd/csrc/wire_group_step.hpp, the functions the grouped
// codec kernels call (wire_group.hip), on the host: tests/test_endpoint_groups.py compares what it
// prints with the model, and runs it under the address and undefined-behaviour sanitizers.
//
//   check_wire_group decode FILE   first line "IB K ring F W stride cases", then per case
//                                  "last start n PACKET COLUMN" (hex, "-" for no bytes)
//                                  -> per case "status decoded newest COLUMN"
//   check_wire_group encode FILE   first line "IB K ring F first_frame stride cases", then per case
//                                  "acked newest COLUMN" -> per case "length start PACKET"
//   check_wire_group fuzz SEED N   N endpoints of random bytes, lengths, start frames and watermarks
//                                  through every instantiation; prints a digest
//
// COLUMN: the endpoint's F frames (ring: slots) of K members of IB bytes each, frame-major.
// Every packet sits in a heap buffer of exactly its bytes, every column in one of exactly F frames;
// an access outside either aborts.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "wire_group_step.hpp"

namespace {

[[noreturn]] void die(const char* what) {
  std::fprintf(stderr, "check_wire_group: %s\n", what);
  std::abort();
}

std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  if (s.size() % 2) die("odd hex");
  auto nib = [](char c) -> int { return c <= '9' ? c - '0' : c - 'a' + 10; };
  for (size_t i = 0; i < s.size(); i += 2) out.push_back(static_cast<uint8_t>(nib(s[i]) * 16 + nib(s[i + 1])));
  return out;
}

std::string hex(const uint8_t* p, size_t n) {
  if (n == 0) return "-";
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) s += d[p[i] >> 4], s += d[p[i] & 15];
  return s;
}

// one endpoint's columns: frames x K members x IB bytes in a buffer of exactly that size
template <int IB, int K>
struct Column {
  std::unique_ptr<uint8_t[]> bytes;
  size_t frames;
  explicit Column(const std::vector<uint8_t>& v, size_t f) : bytes(new uint8_t[v.size()]), frames(f) {
    if (v.size() != f * K * IB) die("column size");
    std::memcpy(bytes.get(), v.data(), v.size());
  }
  uint32_t load(int m, size_t slot) const {
    if (slot >= frames || m < 0 || m >= K) die("load outside the column");
    uint32_t v = 0;
    std::memcpy(&v, bytes.get() + (slot * K + m) * IB, IB);
    return v;
  }
  void store(int m, size_t slot, uint32_t v) {
    if (slot >= frames || m < 0 || m >= K) die("store outside the column");
    std::memcpy(bytes.get() + (slot * K + m) * IB, &v, IB);
  }
};

template <int IB, int K>
struct DecIo {
  Column<IB, K>& col;
  const uint8_t* pk;  // exactly `held` bytes
  int32_t held;
  int64_t stride;
  uint32_t load(int m, size_t slot) { return col.load(m, slot); }
  void store(int m, size_t slot, uint32_t v) { col.store(m, slot, v); }
  void chunk(int32_t off, uint32_t (&w)[4]) {
    if (off < 0 || off % 16 != 0 || off + 16 > stride) die("chunk outside the row");
    uint8_t b[16];
    std::memset(b, 0xA5, 16);  // what the row holds past the packet is noise
    if (off < held) std::memcpy(b, pk + off, static_cast<size_t>(held - off < 16 ? held - off : 16));
    std::memcpy(w, b, 16);
  }
};

template <int IB, int K, bool kRing>
int32_t decode_one(Column<IB, K>& col, int32_t last, int32_t start, int32_t n, const std::vector<uint8_t>& packet,
                   int64_t stride, int32_t frames, int32_t W, int32_t& newest, bool& decoded) {
  const int32_t held = static_cast<int32_t>(packet.size());
  std::unique_ptr<uint8_t[]> exact(new uint8_t[packet.size() ? packet.size() : 1]);
  if (held) std::memcpy(exact.get(), packet.data(), packet.size());
  DecIo<IB, K> io{col, exact.get(), held, stride};
  uint32_t head[8];
  uint32_t lo[4], hi[4];
  io.chunk(0, lo), io.chunk(16, hi);
  for (int i = 0; i < 4; ++i) head[i] = lo[i], head[4 + i] = hi[i];
  return rb::wg_decode<IB, K, kRing>(io, n, start, last, head, stride, frames, W, newest, decoded);
}

template <int IB, int K>
struct EncIo {
  const Column<IB, K>& col;
  uint8_t* row;  // exactly `stride` bytes
  int64_t stride;
  uint32_t load(int m, size_t slot) { return col.load(m, slot); }
  void store_byte(int32_t pos, uint32_t b) {
    if (pos < 32 || pos >= stride) die("byte store outside the row");
    row[pos] = static_cast<uint8_t>(b);
  }
  void store16(int i, const uint32_t (&w)[4]) {
    if (i < 0 || i > 1 || 16 * (i + 1) > stride) die("chunk store outside the row");
    std::memcpy(row + 16 * i, w, 16);
  }
};

template <int IB, int K, bool kRing>
int32_t encode_one(const Column<IB, K>& col, int32_t acked, int32_t newest, int32_t first_frame, int32_t frames,
                   int64_t stride, int32_t& start, std::vector<uint8_t>& row) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[static_cast<size_t>(stride)]);
  std::memset(exact.get(), 0xEE, static_cast<size_t>(stride));
  EncIo<IB, K> io{col, exact.get(), stride};
  const int32_t n = rb::wg_encode<IB, K, kRing>(io, acked, newest, first_frame, frames, stride, start);
  row.assign(exact.get(), exact.get() + stride);
  return n;
}

struct Shape {
  int ib, k, ring;
};

// call f.template operator()<IB, K, kRing>() for the run-time shape
template <class F>
void dispatch(const Shape& s, F&& f) {
#define RB_CASE(IB, K)                                  \
  if (s.ib == IB && s.k == K) {                         \
    if (s.ring) f.template operator()<IB, K, true>();   \
    else f.template operator()<IB, K, false>();         \
    return;                                             \
  }
  RB_CASE(1, 1) RB_CASE(1, 2) RB_CASE(1, 3) RB_CASE(1, 4) RB_CASE(2, 1) RB_CASE(2, 2) RB_CASE(2, 3) RB_CASE(2, 4)
  RB_CASE(4, 1) RB_CASE(4, 2) RB_CASE(4, 3) RB_CASE(4, 4)
#undef RB_CASE
  die("shape");
}

struct DecodeFile {
  std::istream& in;
  Shape s;
  int32_t F, W, cases;
  int64_t stride;
  template <int IB, int K, bool kRing>
  void operator()() {
    for (int32_t c = 0; c < cases; ++c) {
      int32_t last, start, n;
      std::string pk, col;
      if (!(in >> last >> start >> n >> pk >> col)) die("short decode file");
      Column<IB, K> column(unhex(col), static_cast<size_t>(F));
      int32_t newest = 0;
      bool decoded = false;
      const int32_t code = decode_one<IB, K, kRing>(column, last, start, n, unhex(pk), stride, F, W, newest, decoded);
      std::printf("%d %d %d %s\n", code, decoded ? 1 : 0, newest, hex(column.bytes.get(), static_cast<size_t>(F) * K * IB).c_str());
    }
  }
};

struct EncodeFile {
  std::istream& in;
  Shape s;
  int32_t F, first_frame, cases;
  int64_t stride;
  template <int IB, int K, bool kRing>
  void operator()() {
    for (int32_t c = 0; c < cases; ++c) {
      int32_t acked, newest;
      std::string col;
      if (!(in >> acked >> newest >> col)) die("short encode file");
      const Column<IB, K> column(unhex(col), static_cast<size_t>(F));
      int32_t start = 0;
      std::vector<uint8_t> row;
      const int32_t n = encode_one<IB, K, kRing>(column, acked, newest, first_frame, F, stride, start, row);
      std::printf("%d %d %s\n", n, start, hex(row.data(), n > 0 ? static_cast<size_t>(n) : 0).c_str());
    }
  }
};

struct Rng {  // splitmix64
  uint64_t x;
  uint64_t next() {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return static_cast<uint32_t>(next() % n); }
};

struct Fuzz {
  Rng& rng;
  int32_t count;
  uint64_t& digest;
  template <int IB, int K, bool kRing>
  void operator()() {
    const int32_t F = kRing ? 128 : 40, W = 8;
    static const int32_t edges[] = {-2147483647 - 1, -2147483647, -3, -2, -1, 0, 1, 2, 39, 40, 41, 126, 127, 128, 129,
                                    2147483646, 2147483647};
    auto frame = [&]() -> int32_t {
      const uint32_t pick = rng.below(4);
      if (pick == 0) return edges[rng.below(sizeof(edges) / sizeof(edges[0]))];
      if (pick == 1) return static_cast<int32_t>(rng.next());
      return static_cast<int32_t>(rng.below(300)) - 4;
    };
    for (int32_t c = 0; c < count; ++c) {
      const int64_t stride = rng.below(2) ? 32 : 16 * (2 + rng.below(8));
      std::vector<uint8_t> col(static_cast<size_t>(F) * K * IB);
      for (auto& b : col) b = rng.below(4) ? static_cast<uint8_t>(rng.next()) : (rng.below(2) ? 0 : 0xFF);
      // decode: random bytes, biased towards short segment headers so the parse goes deep
      const int32_t held = static_cast<int32_t>(rng.below(static_cast<uint32_t>(stride) + 1));
      std::vector<uint8_t> pk(static_cast<size_t>(held));
      for (auto& b : pk) b = rng.below(3) ? static_cast<uint8_t>(rng.below(32)) : static_cast<uint8_t>(rng.next());
      int32_t n = held;
      if (rng.below(8) == 0) n = frame();  // a length that is not the packet's
      const int32_t last = frame();
      const int32_t start = rng.below(2) ? static_cast<int32_t>(static_cast<int64_t>(last) + 1 - rng.below(3)) : frame();
      Column<IB, K> column(col, static_cast<size_t>(F));
      int32_t newest = 0, st = 0;
      bool decoded = false;
      // a length past what the buffer holds, within the row: the row's bytes there are noise
      const int32_t code = decode_one<IB, K, kRing>(column, last, start, n, pk, stride, F, W, newest, decoded);
      digest = digest * 1099511628211ull + static_cast<uint32_t>(code) + (decoded ? 7u : 0u) + static_cast<uint32_t>(newest);
      // encode
      const int32_t acked = frame();
      const int32_t nw = rng.below(2) ? static_cast<int32_t>(static_cast<int64_t>(acked) + rng.below(140)) : frame();
      std::vector<uint8_t> row;
      const int32_t len = encode_one<IB, K, kRing>(Column<IB, K>(col, static_cast<size_t>(F)), acked, nw,
                                                  static_cast<int32_t>(rng.below(4)), F, stride, st, row);
      if (len > stride || len < -2) die("encode length out of range");
      digest = digest * 1099511628211ull + static_cast<uint32_t>(len) + static_cast<uint32_t>(st);
    }
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) die("usage: decode FILE | encode FILE | fuzz SEED N");
  const std::string mode = argv[1];
  if (mode == "fuzz") {
    if (argc < 4) die("fuzz SEED N");
    Rng rng{std::strtoull(argv[2], nullptr, 10)};
    uint64_t digest = 1469598103934665603ull;
    for (int ib : {1, 2, 4})
      for (int k = 1; k <= 4; ++k)
        for (int ring = 0; ring < 2; ++ring) dispatch(Shape{ib, k, ring}, Fuzz{rng, std::atoi(argv[3]), digest});
    std::printf("fuzz ok %" PRIu64 "\n", digest);
    return 0;
  }
  std::ifstream in(argv[2]);
  if (!in) die("cannot open the file");
  Shape s{};
  int32_t F = 0, x = 0, cases = 0;
  int64_t stride = 0;
  if (!(in >> s.ib >> s.k >> s.ring >> F >> x >> stride >> cases)) die("first line");
  if (mode == "decode") dispatch(s, DecodeFile{in, s, F, x, cases, stride});
  else if (mode == "encode") dispatch(s, EncodeFile{in, s, F, x, cases, stride});
  else die("mode");
  return 0;
}
