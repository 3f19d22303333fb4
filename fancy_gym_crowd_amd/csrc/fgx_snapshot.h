// fgx_snapshot.h — complete engine snapshots: every per-env array a handle keeps between calls
// (DevState q .. start) to / from one device blob, and whole envs copied between rows or handles.
//
// Blob: the sections in DevState order -- q, qd, goal, hole, aux, steps, plans, flags, rng, cond,
// start -- each SoA [rows][N] exactly as the handle holds it, each starting on a 256-byte boundary,
// no header.  A section the handle does not allocate (aux, cond: null in DevState) takes no space.
// rew, plan_len and the tables are not state: per-step scratch, a per-step input, a function of the
// config.  A blob says nothing about where it came from: the caller keeps it with the fingerprint
// (fgx_fingerprint) and n_envs of its handle (include/fgx.h).
#pragma once
#include <string>

#include "fgx_device.h"

namespace fgx {

enum : int { SEC_Q, SEC_QD, SEC_GOAL, SEC_HOLE, SEC_AUX, SEC_STEPS, SEC_PLANS, SEC_FLAGS, SEC_RNG, SEC_COND, SEC_START,
             kSnapSections };
constexpr size_t kSnapAlign = 256;

struct SnapSection {
  size_t offset;   // in the blob (a multiple of kSnapAlign; an absent section: where it would start)
  int rows, elem;  // [rows][N] elements of `elem` bytes
  int bytes_per_env() const { return present ? rows * elem : 0; }
  bool present;
};
struct SnapLayout {
  SnapSection sec[kSnapSections];
  size_t bytes;    // the whole blob: sum over the present sections of bytes_per_env * N rounded up to kSnapAlign
};

// the section's array in a handle
inline char* snap_base(const DevState& s, int k) {
  void* const p[kSnapSections] = {s.q, s.qd, s.goal, s.hole, s.aux, s.steps, s.plans, s.flags, s.rng, s.cond, s.start};
  return (char*)p[k];
}

// Host, no device work: where each section of this handle's blob lies.
inline SnapLayout snapshot_layout(const DevCfg& c, const DevState& s) {
  const int rows[kSnapSections] = {c.nl, c.nl, 2, 3, 3, 1, 1, 1, 5, 2 * c.nl, 1};
  const int elem[kSnapSections] = {8, 8, 8, 8, 8, 4, 4, 4, 8, 4, 8};
  SnapLayout L;
  size_t off = 0;
  for (int k = 0; k < kSnapSections; ++k) {
    const bool present = (k != SEC_AUX && k != SEC_COND) || snap_base(s, k) != nullptr;
    L.sec[k] = {off, rows[k], elem[k], present};
    if (present) off = (off + (size_t)rows[k] * elem[k] * (size_t)c.N + kSnapAlign - 1) & ~(kSnapAlign - 1);
  }
  L.bytes = off;
  return L;
}

// ---------------------------------------------------------------- k_snapshot / k_restore
// One launch moves every section: blockIdx.y is the section, the x dimension strides over its
// 16-byte pieces.  A section's last piece may reach up to 12 bytes past its end: in the blob and in
// the handle alike a section is followed by padding up to the next 256-byte boundary (fgx_create
// lays the state block out that way), so the piece stays inside the allocation and touches no
// other array.
struct SnapCopy {
  const uint4* src[kSnapSections];
  uint4* dst[kSnapSections];
  unsigned n16[kSnapSections];   // 16-byte pieces (0: absent)
};

__device__ __forceinline__ void snap_copy_section(const SnapCopy& p) {
  const int k = blockIdx.y;
  const uint4* __restrict__ src = p.src[k];
  uint4* __restrict__ dst = p.dst[k];
  const unsigned n = p.n16[k], stride = gridDim.x * blockDim.x;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}
__global__ void k_snapshot(SnapCopy p) { snap_copy_section(p); }
__global__ void k_restore(SnapCopy p) { snap_copy_section(p); }

// to_blob: handle -> blob (k_snapshot), else blob -> handle (k_restore).  blob: 16-byte aligned.
inline int snapshot_launch(const DevCfg& c, const DevState& s, char* blob, bool to_blob, hipStream_t stream,
                           std::string& err) {
  const SnapLayout L = snapshot_layout(c, s);
  SnapCopy p = {};
  unsigned most = 0;
  for (int k = 0; k < kSnapSections; ++k) {
    if (!L.sec[k].present) continue;
    const size_t n16 = ((size_t)L.sec[k].bytes_per_env() * (size_t)c.N + 15) / 16;
    if (n16 > 0xffffffffu) { err = "snapshot: a section exceeds 64 GiB"; return -4; }
    uint4* const in_handle = (uint4*)snap_base(s, k);
    uint4* const in_blob = (uint4*)(blob + L.sec[k].offset);
    p.src[k] = to_blob ? in_handle : in_blob;
    p.dst[k] = to_blob ? in_blob : in_handle;
    p.n16[k] = (unsigned)n16;
    most = n16 > most ? (unsigned)n16 : most;
  }
  // one piece per lane for the largest section up to 4096 workgroups per section (1 M envs of 5 links),
  // strided past that; the workgroups beyond a shorter section's end leave at once
  const int threads = 256;
  unsigned blocks = (most + threads - 1) / threads;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  if (to_blob) return launch("k_snapshot", k_snapshot, dim3(blocks, kSnapSections), dim3(threads), 0, stream, err, p);
  return launch("k_restore", k_restore, dim3(blocks, kSnapSections), dim3(threads), 0, stream, err, p);
}

// ---------------------------------------------------------------- k_copy_envs
// For each j < m: every present section's column src_idx[j] of the source goes to column dst_idx[j]
// of the destination (handles of one configuration: the same sections, possibly other env counts).
// One lane handles one (j, row) pair -- a row is one [N] array of 8-byte words (4-byte for steps,
// plans, flags, cond) -- so consecutive lanes touch consecutive j of one row: a fan-out into a
// contiguous range of destinations stores contiguously.
// The caller's contract, which is what makes one pass correct: dst_idx holds distinct envs (src_idx
// may repeat: fan-out), and when source and destination are the same handle no env is in both index
// sets (an env read as a source is never written in the same launch).  A pair with an index outside
// its handle's env range is skipped; nothing outside the arrays is read or written.
struct EnvCopy {
  const char* src[kSnapSections];
  char* dst[kSnapSections];
  int rows[kSnapSections];   // 0: absent
  int elem[kSnapSections];
  int64_t n_src, n_dst;
};

__global__ void k_copy_envs(EnvCopy p, const int64_t* __restrict__ dst_idx, const int64_t* __restrict__ src_idx,
                            int64_t m) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  int k = 0, r = blockIdx.y;   // the row's section (wave-uniform)
  while (r >= p.rows[k]) r -= p.rows[k++];
  const int64_t si = src_idx[j], di = dst_idx[j];
  if ((uint64_t)si >= (uint64_t)p.n_src || (uint64_t)di >= (uint64_t)p.n_dst) return;
  if (p.elem[k] == 8)
    ((uint64_t*)p.dst[k])[(int64_t)r * p.n_dst + di] = ((const uint64_t*)p.src[k])[(int64_t)r * p.n_src + si];
  else
    ((uint32_t*)p.dst[k])[(int64_t)r * p.n_dst + di] = ((const uint32_t*)p.src[k])[(int64_t)r * p.n_src + si];
}

// dst / src: handles of one configuration (fgx_copy_envs checks the fingerprints); m > 0
inline int copy_envs_launch(const DevCfg& cd, const DevState& sd, const DevCfg& cs, const DevState& ss,
                            const int64_t* dst_idx, const int64_t* src_idx, int64_t m, hipStream_t stream,
                            std::string& err) {
  const SnapLayout L = snapshot_layout(cd, sd);
  EnvCopy p = {};
  int total_rows = 0;
  for (int k = 0; k < kSnapSections; ++k) {
    const bool both = L.sec[k].present && snap_base(ss, k) != nullptr;
    p.src[k] = snap_base(ss, k);
    p.dst[k] = snap_base(sd, k);
    p.rows[k] = both ? L.sec[k].rows : 0;
    p.elem[k] = L.sec[k].elem;
    total_rows += p.rows[k];
  }
  p.n_src = cs.N;
  p.n_dst = cd.N;
  const int threads = 256;
  const int64_t blocks = (m + threads - 1) / threads;
  if (blocks > 0x7fffffff) { err = "k_copy_envs: too many pairs"; return -4; }
  return launch("k_copy_envs", k_copy_envs, dim3((unsigned)blocks, total_rows), dim3(threads), 0, stream, err, p, dst_idx,
                src_idx, m);
}

}  // namespace fgx
