// ggrs_amd/csrc/restart.hpp — the initial values of a batch's per-session buffers
// and the kernel that writes them (include/ggrs_amd.h rb_p2p_restart_sessions,
// rb_spectator_restart_sessions).
//
// Every piece of per-session state is a column of some plane: rows of Spad (or
// Spad * lanes) elements, a session's value at its own column of every row.  A
// PlaneSet lists a batch's planes with what a fresh column holds; the engines
// describe each buffer group in one function (p2p_engine.hip *_planes,
// spectator_engine.hip spectator_planes).  That function is the only
// description of a per-session buffer: run with `make` set it allocates every
// buffer that does not exist yet, through the batch's owner (host_batch.hpp),
// with the extent the plane's own shape gives, so the size restart_kernel and
// the move kernels write by is the size that was allocated.  restart_kernel
// then runs over the set
//   - for every column when the group's buffers are made (create,
//     rb_p2p_time_sync_enable, the first paced tick, the first export), and
//   - for the selected sessions' columns in a restart,
// so a restarted session holds what a created one does by construction: there
// is no second list of initial values or of sizes.
//
// restart_kernel is game independent.  It is defined in the one translation
// unit that sets RB_RESTART_DEFINE (p2p_engine.hip); the others link to
// restart_launch.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "host_batch.hpp"

namespace rb {

// One plane.  Its rows are `groups` groups of `rows_in` rows: row r lies at
//   base + (r / rows_in) * group_stride + (r % rows_in) * stride          (bytes)
// and holds `cps` elements of `esize` bytes per session, session s at columns s * cps + l.
// A fresh column is the byte `fill` repeated, or, with `src`, the template
//   src[((r % rows_in) * src_cols + (src_cols == 1 ? 0 : l)) * esize ...]
// in device memory: one value per row (src_cols 1) or a whole column of lanes (src_cols = cps),
// the same for every group.
struct RestartPlane {
  char* base;
  const char* src;
  unsigned long long stride, group_stride;
  uint32_t rows_in, groups;
  uint32_t chunk0;  // the plane's first row chunk (blockIdx.y), set by restart_launch
  uint8_t esize, cps, src_cols, fill;
};

constexpr int kRestartMaxPlanes = 40, kRestartMaxChunks = 256;
constexpr uint32_t kRestartRows = 16;  // rows per thread, at least

struct RestartTable {
  RestartPlane p[kRestartMaxPlanes];
  uint8_t plane_of[kRestartMaxChunks];  // the plane of row chunk blockIdx.y
  const int32_t* idx;                   // [n] the selected sessions; nullptr: sessions 0 .. n-1
  uint32_t n, rows_per;                 // rows per thread
};

// Every byte of `mask` [n] that is not zero, in order (eight bytes at a time: a restart selects few).
inline void restart_selected(const uint8_t* mask, int n, std::vector<int32_t>& idx) {
  int s = 0;
  for (; s + 8 <= n; s += 8) {
    uint64_t w;
    std::memcpy(&w, mask + s, 8);
    if (!w) continue;
    for (int k = 0; k < 8; ++k)
      if (mask[s + k]) idx.push_back(s + k);
  }
  for (; s < n; ++s)
    if (mask[s]) idx.push_back(s);
}

// A batch's planes under construction: the descriptors, and the template words they refer to by
// offset until bind() points them into the device copy of `tmpl`.
//
// A plane has one of three kinds.  Most have a fresh value, which create and restart write and a
// move (migrate.hpp) carries.  A carry-only plane has none: its stale content is harmless to a
// fresh session (entries behind a count or a NULL frame are never read), so it is listed only when
// `carry` is set, which a move does and create and restart do not: restart_kernel's table is what
// it was.  A fresh-on-move plane is written by create and restart but not carried: the record holds
// its fresh value (a fill byte), so an imported session has it as a restarted one does.
enum : uint8_t { kPlaneFresh = 0, kPlaneCarryOnly = 1, kPlaneFreshOnMove = 2 };

struct PlaneSet {
  size_t Spad = 0;
  bool carry = false;        // list the carry-only planes too
  bool layout_only = false;  // list the groups a later call makes as well, with no buffers: for a record's layout
  DeviceOwner* make = nullptr;  // allocate the listed buffers that do not exist yet
  hipError_t err = hipSuccess;  // the first allocation that failed
  std::vector<RestartPlane> planes;
  std::vector<uint8_t> kind;  // per plane
  std::vector<uint32_t> tmpl;
  std::vector<size_t> tmpl_off;  // per plane: byte offset into tmpl, or npos

  static constexpr size_t npos = ~size_t{0};

  // The extent of one buffer: [rows][Spad * cps] elements.  Every function below that takes a
  // buffer by reference declares it so, from the shape it lists; a buffer that several planes share,
  // or that none lists, is declared here once, by its group function.
  template <class T>
  void buffer(T*& p, int esize, size_t rows, int cps) {
    if (make && !p && err == hipSuccess) err = make->alloc(p, rows * Spad * cps * esize);
  }
  // rows [rows][Spad * cps] at `base`, inside a declared buffer
  void plane(void* base, int esize, size_t rows, int cps, uint8_t fill_byte) {
    RestartPlane q{};
    q.base = static_cast<char*>(base);
    q.stride = static_cast<unsigned long long>(Spad) * cps * esize;
    q.group_stride = q.stride * rows;
    q.rows_in = static_cast<uint32_t>(rows);
    q.groups = 1;
    q.esize = static_cast<uint8_t>(esize);
    q.cps = static_cast<uint8_t>(cps);
    q.src_cols = 1;
    q.fill = fill_byte;
    planes.push_back(q);
    kind.push_back(kPlaneFresh);
    tmpl_off.push_back(npos);
  }
  // [rows][Spad * cps] elements, every fresh element the byte `fill_byte` repeated
  template <class T>
  void fill(T*& base, int esize, size_t rows, int cps, uint8_t fill_byte) {
    buffer(base, esize, rows, cps);
    plane(base, esize, rows, cps, fill_byte);
  }
  // [rows][Spad * cps] elements with no fresh value: carried by a move, skipped otherwise
  template <class T>
  void carried(T*& base, int esize, size_t rows, int cps) {
    buffer(base, esize, rows, cps);
    if (!carry) return;
    plane(base, esize, rows, cps, 0);
    kind.back() = kPlaneCarryOnly;
  }
  // the last plane (a fill) is not carried by a move: the record holds its fresh value
  void fresh_on_move() { kind.back() = kPlaneFreshOnMove; }
  // [groups][rows][Spad] words, row r of every group `values[r]`
  void row_values(int32_t*& base, size_t groups, const std::vector<int32_t>& values) {
    buffer(base, 4, groups * values.size(), 1);
    plane(base, 4, values.size(), 1, 0);
    planes.back().groups = static_cast<uint32_t>(groups);
    tmpl_off.back() = tmpl.size() * 4;
    for (int32_t v : values) tmpl.push_back(static_cast<uint32_t>(v));
  }
  // State planes (word_index) of `cells` cells of NW words for Spad * L lane columns:
  // zero, or with `w0` ([L][NW], GameOps::init_words) that state in every session.
  void state(uint32_t*& base, int NW, int L, size_t cells, const uint32_t* w0) {
    buffer(base, 4, cells * NW, L);
    const size_t Gp = Spad * L, cell_bytes = static_cast<size_t>(NW) * Gp * 4;
    const int Q4 = NW / 4, R = NW % 4;
    size_t t0 = npos;
    if (w0) {  // the template: the planes of a one-session batch, 16-byte aligned
      tmpl.resize((tmpl.size() + 3) / 4 * 4);
      t0 = tmpl.size();
      tmpl.resize(t0 + static_cast<size_t>(NW) * L);
      for (int l = 0; l < L; ++l)
        for (int k = 0; k < NW; ++k) tmpl[t0 + word_index(NW, L, l, k)] = w0[l * NW + k];
    }
    auto part = [&](size_t word0, int esize, size_t rows) {  // word0: the part's first word per column
      plane(base + word0 * Gp, esize, rows, L, 0);
      planes.back().groups = static_cast<uint32_t>(cells);
      planes.back().group_stride = cell_bytes;
      if (w0) {
        planes.back().src_cols = static_cast<uint8_t>(L);
        tmpl_off.back() = (t0 + word0 * L) * 4;
      }
    };
    if (Q4) part(0, 16, Q4);
    if (R >= 2) part(static_cast<size_t>(Q4) * 4, 8, 1);
    if (R & 1) part(static_cast<size_t>(Q4) * 4 + (R >= 2 ? 2 : 0), 4, 1);
  }
  // templates -> device addresses
  void bind(const uint32_t* tmpl_dev) {
    for (size_t i = 0; i < planes.size(); ++i)
      if (tmpl_off[i] != npos) planes[i].src = reinterpret_cast<const char*>(tmpl_dev) + tmpl_off[i];
  }
};

// The selected sessions on their way to the device without a host synchronisation: two pinned
// staging slots, each written again only once the copy that read it has completed (an event per
// slot; the host waits only when it is two restarts ahead of the device), and one device list,
// which the stream orders between the kernels that read it.  Made by the first upload, through `res`.
struct RestartIndex {
  int32_t* host[2] = {nullptr, nullptr};  // [capacity] each, pinned
  int32_t* dev = nullptr;                 // [capacity]
  hipEvent_t done[2] = {nullptr, nullptr};
  bool armed[2] = {false, false};  // done[k] has been recorded
  int next = 0;

  hipError_t upload(DeviceOwner& res, const std::vector<int32_t>& idx, size_t capacity, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (!done[1]) {  // (a partial failure is made again from its first missing piece)
      if (!dev) e = res.alloc(dev, capacity * 4);
      for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        if (!host[k]) e = res.alloc_host(host[k], capacity * 4);
        if (e == hipSuccess && !done[k]) e = res.event(done[k], hipEventDisableTiming);
      }
      if (e != hipSuccess) return e;
    }
    const int k = next;
    if (armed[k] && (e = hipEventSynchronize(done[k])) != hipSuccess) return e;
    std::memcpy(host[k], idx.data(), idx.size() * 4);
    if ((e = hipMemcpyAsync(dev, host[k], idx.size() * 4, hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if ((e = hipEventRecord(done[k], stream)) != hipSuccess) return e;
    armed[k] = true;
    next = k ^ 1;
    return hipSuccess;
  }
};

// restart_kernel over `set` (bound, without carry-only planes) for the n sessions idx[0..n) (device memory; nullptr: 0..n-1).
// One launch, stream ordered.  hipErrorInvalidValue: more than kRestartMaxPlanes planes.
hipError_t restart_launch(const PlaneSet& set, const int32_t* idx, uint32_t n, hipStream_t stream);

#ifdef RB_RESTART_DEFINE
// Rows [r0, r1) of one lane column
template <class T>
__device__ inline void restart_rows(const RestartPlane& q, size_t col, uint32_t l, uint32_t r0, uint32_t r1) {
  const T* __restrict__ src = reinterpret_cast<const T*>(q.src);
  const uint32_t sl = q.src_cols == 1 ? 0u : l;
  const uint32_t w = q.fill * 0x01010101u;
  T blank;
  if constexpr (sizeof(T) == 16) blank = T{w, w, w, w};
  else if constexpr (sizeof(T) == 8) blank = T{w, w};
  else blank = static_cast<T>(w);
  uint32_t g = r0 / q.rows_in, ri = r0 % q.rows_in;
  for (uint32_t r = r0; r < r1; ++r, ++ri) {
    if (ri == q.rows_in) {
      ri = 0;
      ++g;
    }
    const T v = src ? src[static_cast<size_t>(ri) * q.src_cols + sl] : blank;
    *reinterpret_cast<T*>(q.base + static_cast<size_t>(g) * q.group_stride + static_cast<size_t>(ri) * q.stride +
                          col * sizeof(T)) = v;
  }
}

// Thread (j, row chunk): lane column idx[j / cps] * cps + j % cps of rows_per rows of one plane, so a
// session's lanes are consecutive threads and the work is the selected columns only.  blockIdx.y
// walks the row chunks of all planes.  Plain stores; no thread reads what another writes.
__global__ void __launch_bounds__(256) restart_kernel(const RestartTable t) {
  const RestartPlane& q = t.p[t.plane_of[blockIdx.y]];
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= t.n * q.cps) return;
  const uint32_t sj = j / q.cps, l = j % q.cps;
  const size_t col = static_cast<size_t>(t.idx ? static_cast<uint32_t>(t.idx[sj]) : sj) * q.cps + l;
  const uint32_t rows = q.rows_in * q.groups, r0 = (blockIdx.y - q.chunk0) * t.rows_per;
  const uint32_t r1 = r0 + t.rows_per < rows ? r0 + t.rows_per : rows;
  switch (q.esize) {
    case 1: restart_rows<uint8_t>(q, col, l, r0, r1); break;
    case 2: restart_rows<uint16_t>(q, col, l, r0, r1); break;
    case 4: restart_rows<uint32_t>(q, col, l, r0, r1); break;
    case 8: restart_rows<uint2>(q, col, l, r0, r1); break;
    default: restart_rows<uint4>(q, col, l, r0, r1); break;
  }
}

hipError_t restart_launch(const PlaneSet& set, const int32_t* idx, uint32_t n, hipStream_t stream) {
  if (n == 0 || set.planes.empty()) return hipSuccess;
  if (set.planes.size() > static_cast<size_t>(kRestartMaxPlanes) || set.carry) return hipErrorInvalidValue;
  RestartTable t{};
  uint32_t chunks = 0, cps = 1;
  for (t.rows_per = kRestartRows;; t.rows_per *= 2) {  // more rows per thread until the chunks fit the table
    chunks = 0;
    for (const RestartPlane& q : set.planes) chunks += (q.rows_in * q.groups + t.rows_per - 1) / t.rows_per;
    if (chunks <= static_cast<uint32_t>(kRestartMaxChunks)) break;
  }
  chunks = 0;
  for (size_t i = 0; i < set.planes.size(); ++i) {
    t.p[i] = set.planes[i];
    t.p[i].chunk0 = chunks;
    const uint32_t mine = (t.p[i].rows_in * t.p[i].groups + t.rows_per - 1) / t.rows_per;
    for (uint32_t c = 0; c < mine; ++c) t.plane_of[chunks + c] = static_cast<uint8_t>(i);
    chunks += mine;
    if (t.p[i].cps > cps) cps = t.p[i].cps;
  }
  t.idx = idx;
  t.n = n;
  const uint64_t cols = static_cast<uint64_t>(n) * cps;
  if (cols > (1ull << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(restart_kernel, dim3(static_cast<unsigned>((cols + 255) / 256), chunks), dim3(256), 0, stream, t);
  return hipGetLastError();
}
#endif  // RB_RESTART_DEFINE

}  // namespace rb
