// ggrs_amd/csrc/migrate.hpp — moving running sessions between batches
// (include/ggrs_amd.h rb_p2p_export_sessions, rb_p2p_import_sessions,
// rb_spectator_export_sessions, rb_spectator_import_sessions; DESIGN.md
// section 15).
//
// GGRS has no such call: a P2PSession is an ordinary movable Rust value, and
// moving it between two collections is a move of that value.  Here a session
// is a column of every plane of its batch, so the move is a gather of the
// selected columns into session records (session_record.hpp) and a scatter of
// records into the selected columns of another batch, or of the same one.
//
// Both kernels are game independent and read the batch's one list of planes
// (restart.hpp PlaneSet, with the carry-only planes).  They use
// restart_kernel's mapping: thread (j, row chunk) handles lane column
// idx[j / cps] * cps + j % cps of a chunk of rows of one plane, so the work is
// the selected columns only.  They are defined in the translation unit that
// sets RB_RESTART_DEFINE; the others link to move_launch.
#pragma once
#include "restart.hpp"
#include "session_record.hpp"

namespace rb {

// One plane of a move: RestartPlane's addressing, and where its part lies in a record
struct MovePlane {
  char* base;
  unsigned long long stride, group_stride;
  unsigned long long rec_off;
  uint32_t rows_in, groups;
  uint32_t chunk0;  // the plane's first row chunk (blockIdx.y)
  uint8_t esize, cps;
  uint8_t fresh;  // kPlaneFreshOnMove: the gather stores `fill`, not the column
  uint8_t fill;
};

constexpr int kMoveMaxPlanes = 48;  // 48 x 48 bytes + the chunk map: 2.6 KiB of the 4 KiB of kernel arguments

struct MoveTable {
  MovePlane p[kMoveMaxPlanes];
  uint8_t plane_of[kRestartMaxChunks];  // the plane of row chunk blockIdx.y
  const int32_t* idx;                   // [n] the selected sessions: record k is session idx[k]
  char* records;                        // [n][record_bytes]
  unsigned long long record_bytes, fingerprint;
  uint32_t* refused;  // scatter: += 1 per record whose header does not match
  uint32_t n, rows_per;
};

inline std::vector<PlaneShape> plane_shapes(const PlaneSet& set) {
  std::vector<PlaneShape> out;
  for (const RestartPlane& q : set.planes) out.push_back(PlaneShape{q.esize, q.rows_in, q.groups, q.cps});
  return out;
}

// n distinct indices in [0, S): record k belongs to sessions[k]
inline bool move_indices_ok(const int32_t* sessions, int32_t n, int32_t S) {
  if (n < 0 || n > S) return false;
  std::vector<uint8_t> seen(static_cast<size_t>(S), 0);
  for (int32_t k = 0; k < n; ++k) {
    const int32_t s = sessions[k];
    if (s < 0 || s >= S || seen[s]) return false;
    seen[s] = 1;
  }
  return true;
}

// session_gather_kernel (scatter false) or session_scatter_kernel over `set` (listed with carry) for the
// n sessions idx[0..n) (device memory) and the n records at `records` (device memory, 16-byte
// aligned).  One launch, stream ordered.  hipErrorInvalidValue: more than kMoveMaxPlanes planes.
hipError_t move_launch(const PlaneSet& set, const RecordLayout& lay, const int32_t* idx, uint32_t n, void* records,
                       bool scatter, uint32_t* refused, hipStream_t stream);

#ifdef RB_RESTART_DEFINE
// Rows [r0, r1) of one lane column, four loads in flight before their stores (in scalars: an indexed
// array here is an alloca, which the compiler moves to LDS).
template <class T, bool kScatter>
__device__ inline void move_rows(const MovePlane& q, char* rec, size_t col, uint32_t l, uint32_t r0, uint32_t r1) {
  const uint32_t w = q.fill * 0x01010101u;
  T blank;
  if constexpr (sizeof(T) == 16) blank = T{w, w, w, w};
  else if constexpr (sizeof(T) == 8) blank = T{w, w};
  else blank = static_cast<T>(w);
  const size_t cps = q.cps;
  T* rp = reinterpret_cast<T*>(rec + q.rec_off) + static_cast<size_t>(r0) * cps + l;
  uint32_t g = r0 / q.rows_in, ri = r0 % q.rows_in;
  auto next = [&]() -> T* {  // the column's element in the next row of the plane
    T* p = reinterpret_cast<T*>(q.base + static_cast<size_t>(g) * q.group_stride + static_cast<size_t>(ri) * q.stride +
                                col * sizeof(T));
    if (++ri == q.rows_in) {
      ri = 0;
      ++g;
    }
    return p;
  };
  const bool fresh = !kScatter && q.fresh;
  for (uint32_t r = r0; r < r1; r += 4, rp += 4 * cps) {
    const uint32_t m = r1 - r;  // rows left: rows past them are neither read nor written
    T* const p0 = next();
    T* const p1 = next();
    T* const p2 = next();
    T* const p3 = next();
    T* const s0 = kScatter ? rp : p0;  // from
    T* const s1 = kScatter ? rp + cps : p1;
    T* const s2 = kScatter ? rp + 2 * cps : p2;
    T* const s3 = kScatter ? rp + 3 * cps : p3;
    T v0 = blank, v1 = blank, v2 = blank, v3 = blank;
    if (!fresh) {
      v0 = *s0;
      if (m > 1) v1 = *s1;
      if (m > 2) v2 = *s2;
      if (m > 3) v3 = *s3;
    }
    T* const d0 = kScatter ? p0 : rp;  // to
    T* const d1 = kScatter ? p1 : rp + cps;
    T* const d2 = kScatter ? p2 : rp + 2 * cps;
    T* const d3 = kScatter ? p3 : rp + 3 * cps;
    *d0 = v0;
    if (m > 1) *d1 = v1;
    if (m > 2) *d2 = v2;
    if (m > 3) *d3 = v3;
  }
}

template <bool kScatter>
__device__ inline void move_body(const MoveTable& t) {
  const MovePlane& q = t.p[t.plane_of[blockIdx.y]];
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t.n * q.cps) return;
  const uint32_t sj = j / q.cps, l = j % q.cps;
  char* const rec = t.records + static_cast<size_t>(sj) * t.record_bytes;
  const bool first = blockIdx.y == 0 && l == 0;  // one thread per record
  if constexpr (kScatter) {
    // every thread of a record reads the same header, which nothing writes: they decide alike
    const uint4 h0 = *reinterpret_cast<const uint4*>(rec), h1 = *reinterpret_cast<const uint4*>(rec + 16);
    const bool ok = h0.x == kRecordMagic && h0.y == kRecordVersion && h0.z == static_cast<uint32_t>(t.record_bytes) &&
                    h0.w == static_cast<uint32_t>(t.record_bytes >> 32) && h1.x == static_cast<uint32_t>(t.fingerprint) &&
                    h1.y == static_cast<uint32_t>(t.fingerprint >> 32);
    if (!ok) {
      if (first) atomicAdd(t.refused, 1u);
      return;
    }
  } else if (first) {
    *reinterpret_cast<uint4*>(rec) = uint4{kRecordMagic, kRecordVersion, static_cast<uint32_t>(t.record_bytes),
                                           static_cast<uint32_t>(t.record_bytes >> 32)};
    *reinterpret_cast<uint4*>(rec + 16) =
        uint4{static_cast<uint32_t>(t.fingerprint), static_cast<uint32_t>(t.fingerprint >> 32), 0u, 0u};
  }
  const size_t col = static_cast<size_t>(static_cast<uint32_t>(t.idx[sj])) * q.cps + l;
  const uint32_t rows = q.rows_in * q.groups, r0 = (blockIdx.y - q.chunk0) * t.rows_per;
  const uint32_t r1 = r0 + t.rows_per < rows ? r0 + t.rows_per : rows;
  switch (q.esize) {
    case 1: move_rows<uint8_t, kScatter>(q, rec, col, l, r0, r1); break;
    case 2: move_rows<uint16_t, kScatter>(q, rec, col, l, r0, r1); break;
    case 4: move_rows<uint32_t, kScatter>(q, rec, col, l, r0, r1); break;
    case 8: move_rows<uint2, kScatter>(q, rec, col, l, r0, r1); break;
    default: move_rows<uint4, kScatter>(q, rec, col, l, r0, r1); break;
  }
}

// The selected columns of every plane -> records.  Plain loads and stores of the plane's element
// size; no thread reads what another writes; the source is only read.
__global__ void __launch_bounds__(256) session_gather_kernel(const MoveTable t) { move_body<false>(t); }

// Records -> the selected columns.  A record whose header is not the destination's (magic, version,
// record_bytes, fingerprint) leaves its column untouched, in every plane, and counts once.
__global__ void __launch_bounds__(256) session_scatter_kernel(const MoveTable t) { move_body<true>(t); }

hipError_t move_launch(const PlaneSet& set, const RecordLayout& lay, const int32_t* idx, uint32_t n, void* records,
                       bool scatter, uint32_t* refused, hipStream_t stream) {
  if (n == 0 || set.planes.empty()) return hipSuccess;
  if (set.planes.size() > static_cast<size_t>(kMoveMaxPlanes) || lay.off.size() != set.planes.size())
    return hipErrorInvalidValue;
  MoveTable t{};
  uint32_t chunks = 0, cps = 1;
  for (t.rows_per = kRestartRows;; t.rows_per *= 2) {  // more rows per thread until the chunks fit the table
    chunks = 0;
    for (const RestartPlane& q : set.planes) chunks += (q.rows_in * q.groups + t.rows_per - 1) / t.rows_per;
    if (chunks <= static_cast<uint32_t>(kRestartMaxChunks)) break;
  }
  chunks = 0;
  for (size_t i = 0; i < set.planes.size(); ++i) {
    const RestartPlane& s = set.planes[i];
    MovePlane& q = t.p[i];
    q.base = s.base;
    q.stride = s.stride;
    q.group_stride = s.group_stride;
    q.rec_off = lay.off[i];
    q.rows_in = s.rows_in;
    q.groups = s.groups;
    q.esize = s.esize;
    q.cps = s.cps;
    q.fresh = set.kind[i] == kPlaneFreshOnMove;
    q.fill = s.fill;
    q.chunk0 = chunks;
    const uint32_t mine = (s.rows_in * s.groups + t.rows_per - 1) / t.rows_per;
    for (uint32_t c = 0; c < mine; ++c) t.plane_of[chunks + c] = static_cast<uint8_t>(i);
    chunks += mine;
    if (s.cps > cps) cps = s.cps;
  }
  t.idx = idx;
  t.records = static_cast<char*>(records);
  t.record_bytes = lay.record_bytes;
  t.fingerprint = lay.fingerprint;
  t.refused = refused;
  t.n = n;
  const uint64_t cols = static_cast<uint64_t>(n) * cps;
  if (cols > (1ull << 31)) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>((cols + 255) / 256), chunks), block(256);
  if (scatter) hipLaunchKernelGGL(session_scatter_kernel, grid, block, 0, stream, t);
  else hipLaunchKernelGGL(session_gather_kernel, grid, block, 0, stream, t);
  return hipGetLastError();
}
#endif  // RB_RESTART_DEFINE

// ---- The restart and the move of a P2P or a spectator batch B, written once.  B has S, Spad,
// device, stream, res, tmpl / tmpl_host (the templates of create), restart_idx, move_idx, refused,
// and says what differs: kApi (the entry points' prefix in messages), planes(ps) (every plane
// group it has), record_config() (the words its kernels compile in or read: a record goes only
// into a batch that agrees) and before_move() (the groups a later call would make).

// idx: the selected sessions (empty with a null mask: all of them)
template <class B>
rb_status restart_sessions(B* b, const uint8_t* session_mask, std::vector<int32_t>& idx) {
  if (session_mask) {
    restart_selected(session_mask, b->S, idx);
    if (idx.empty()) return RB_OK;
  }
  const bool all = !session_mask || idx.size() == static_cast<size_t>(b->S);
  DeviceScope dev_scope(b->device);
  PlaneSet ps;
  ps.Spad = static_cast<size_t>(b->Spad);
  b->planes(ps);
  if (ps.tmpl != b->tmpl_host)
    return fail(b, RB_DEVICE_ERROR, std::string(B::kApi) + "_restart_sessions: the templates moved since create");
  ps.bind(b->tmpl);
  if (!all) RB_TRY(b, b->restart_idx.upload(b->res, idx, static_cast<size_t>(b->S), b->stream));
  RB_TRY(b, restart_launch(ps, all ? nullptr : b->restart_idx.dev, static_cast<uint32_t>(all ? b->S : idx.size()), b->stream));
  return RB_OK;
}

// Every per-session plane the batch's configuration can have, the carry-only ones included.
// layout_only: without making the lazily made groups (their planes have no buffers).
template <class B>
RecordLayout record_planes(B* b, PlaneSet& ps, bool layout_only) {
  ps.Spad = static_cast<size_t>(b->Spad);
  ps.carry = true;
  ps.layout_only = layout_only;
  b->planes(ps);
  return record_layout(plane_shapes(ps), b->record_config());
}

template <class B>
rb_status move_sessions(B* b, const int32_t* sessions, int32_t n, void* records, bool scatter) {
  const std::string who = std::string(B::kApi) + (scatter ? "_import_sessions" : "_export_sessions");
  if (n < 0 || (n > 0 && (!sessions || !records))) return fail(b, RB_INVALID_REQUEST, who + ": missing session list or records");
  if (!move_indices_ok(sessions, n, b->S))
    return fail(b, RB_INVALID_REQUEST, who + ": sessions must be distinct indices in [0, num_sessions)");
  if (n == 0) return RB_OK;
  if (reinterpret_cast<uintptr_t>(records) % 16 != 0) return fail(b, RB_INVALID_REQUEST, who + ": records need 16-byte alignment");
  DeviceScope dev_scope(b->device);
  if (const rb_status r = b->before_move(); r != RB_OK) return r;
  if (scatter && !b->refused) {  // made by the first import
    RB_TRY(b, b->res.alloc(b->refused, 4));
    RB_TRY(b, hipMemsetAsync(b->refused, 0, 4, b->stream));
  }
  PlaneSet ps;
  const RecordLayout lay = record_planes(b, ps, false);
  RB_TRY(b, b->move_idx.upload(b->res, std::vector<int32_t>(sessions, sessions + n), static_cast<size_t>(b->S), b->stream));
  RB_TRY(b, move_launch(ps, lay, b->move_idx.dev, static_cast<uint32_t>(n), records, scatter, b->refused, b->stream));
  return RB_OK;
}

template <class B>
rb_status import_refused(B* b, uint32_t* count) {
  if (!count) return RB_OK;
  *count = 0;
  if (!b->refused) return RB_OK;  // no import yet
  DeviceScope dev_scope(b->device);
  RB_TRY(b, hipMemcpyAsync(count, b->refused, 4, hipMemcpyDeviceToHost, b->stream));
  RB_TRY(b, hipStreamSynchronize(b->stream));
  return RB_OK;
}

}  // namespace rb
