// ggrs_amd/csrc/session_record.hpp — the layout of a session record
// (include/ggrs_amd.h rb_p2p_export_sessions, rb_p2p_import_sessions and the
// spectators' twins).
//
// A record is a position-independent byte image of one session: a header and
// then every per-session plane of its batch (restart.hpp PlaneSet, the
// carry-only planes included), in table order.  Plane i's part holds the
// session's column of that plane, row major with the lanes innermost:
//   element (row r, lane l) at  off[i] + (r * cps + l) * esize      (bytes)
// for r in [0, rows_in * groups), so a session's lanes store consecutive
// elements.  Every part starts at a multiple of its element size and
// record_bytes is a multiple of 16: with a 16-byte aligned buffer of records
// every element is naturally aligned.  Bytes between parts are padding and are
// never read.
//
// Plain C++: a host program can include this file and check the layout
// (tests/check_session_record.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rb {

constexpr uint32_t kRecordMagic = 0x53524252u;  // "RBRS"
constexpr uint32_t kRecordVersion = 1;

// The first bytes of every record.  The scatter compares all of it with what the destination
// batch expects before it writes anything.
struct RecordHeader {
  uint32_t magic, version;
  uint64_t record_bytes;
  uint64_t fingerprint;
  uint64_t reserved;  // 0
};
static_assert(sizeof(RecordHeader) == 32, "two 16-byte loads");
constexpr size_t kRecordHeaderBytes = sizeof(RecordHeader);

// What of a plane the layout depends on (restart.hpp RestartPlane)
struct PlaneShape {
  uint32_t esize, rows_in, groups, cps;
};

struct RecordLayout {
  std::vector<size_t> off;  // per plane: its part's first byte
  size_t record_bytes = 0;
  uint64_t fingerprint = 0;
};

// The state planes' layout, for `cols` lane columns: a column's NW words lie in groups of four
// (16-byte elements), then a pair (8 bytes), then a single word.  Word k of column c.  The same
// function gives the layout of a one-session batch, the form a live state's template is kept in.
inline size_t word_index(int NW, size_t cols, size_t c, int k) {
  const int Q4 = NW / 4, R = NW % 4;
  if (k < Q4 * 4) return static_cast<size_t>(k / 4) * 4 * cols + c * 4 + (k % 4);
  size_t b = static_cast<size_t>(Q4) * 4 * cols;
  if (R >= 2) {
    if (k < Q4 * 4 + 2) return b + c * 2 + (k - Q4 * 4);
    b += 2 * cols;
  }
  return b + c;
}

inline uint64_t record_hash_word(uint64_t h, uint32_t w) {  // FNV-1a, a byte at a time
  for (int i = 0; i < 4; ++i) {
    h ^= (w >> (8 * i)) & 0xffu;
    h *= 0x100000001b3ull;
  }
  return h;
}

inline size_t plane_part_bytes(const PlaneShape& q) {
  return static_cast<size_t>(q.rows_in) * q.groups * q.cps * q.esize;
}

// The parts' offsets, the record's size and the fingerprint: a hash of the plane list (element
// size, rows, groups and columns per session of each plane, in table order) and of `config`, the
// words of the batch's configuration that its kernels compile in or read.
inline RecordLayout record_layout(const std::vector<PlaneShape>& planes, const std::vector<uint32_t>& config) {
  RecordLayout out;
  size_t at = kRecordHeaderBytes;
  uint64_t h = 0xcbf29ce484222325ull;
  h = record_hash_word(h, static_cast<uint32_t>(planes.size()));
  for (const PlaneShape& q : planes) {
    at = (at + q.esize - 1) / q.esize * q.esize;
    out.off.push_back(at);
    at += plane_part_bytes(q);
    h = record_hash_word(h, q.esize);
    h = record_hash_word(h, q.rows_in);
    h = record_hash_word(h, q.groups);
    h = record_hash_word(h, q.cps);
  }
  h = record_hash_word(h, static_cast<uint32_t>(config.size()));
  for (uint32_t w : config) h = record_hash_word(h, w);
  out.record_bytes = (at + 15) / 16 * 16;
  out.fingerprint = h;
  return out;
}

}  // namespace rb
