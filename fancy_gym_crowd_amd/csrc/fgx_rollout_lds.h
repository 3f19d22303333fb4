// fgx_rollout_lds.h — LDS sizing of k_rollout_raw (fgx_rollout.h), stated once for the kernel and
// for the host that launches it; plain C++, so tests/host/rollout_lds_check.hip compiles it alone.
//
// Each wave of the workgroup stages the action rows of its own 64 envs: a chunk of
// rollout_chunk(dof) steps, [step][env][dof] with the odd row stride of k_step_raw
// (step_raw_stride), and at the end the envs' observation rows in the same region.  The chunk is
// the largest that keeps a workgroup of four waves within 1/8 of a CU's 160 KiB of LDS, the share
// of one workgroup at the most waves a SIMD holds (8), so the action staging never caps
// occupancy; the observation rows (up to 29 floats per env at 8 links) allow 5 workgroups per CU,
// above what the kernel's registers admit.
#pragma once

#ifndef FGX_HD   // (as fgx_npsum.h)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define FGX_HD __host__ __device__
#else
#define FGX_HD
#endif
#endif

namespace fgx {
constexpr int kRolloutBlock = 256;                      // threads of a workgroup: four waves, 256 consecutive envs
constexpr int kRolloutWaves = kRolloutBlock / 64;
constexpr int kRolloutLaneFloats = 20;                  // 160 KiB / 8 workgroups / 256 lanes / 4 B
FGX_HD constexpr int rollout_stride(int w) { return w | 1; }   // odd LDS row stride (= step_raw_stride)
// steps of actions a wave stages at once
FGX_HD constexpr int rollout_chunk(int dof) {
  const int k = kRolloutLaneFloats / rollout_stride(dof);
  return k < 1 ? 1 : (k > 16 ? 16 : k);
}
// floats of one wave's region; obs_dim: the width of the observation rows leaving through it (0: none)
FGX_HD constexpr int rollout_wave_floats(int dof, int obs_dim) {
  const int a = rollout_chunk(dof) * 64 * rollout_stride(dof);
  const int o = obs_dim > 0 ? 64 * rollout_stride(obs_dim) : 0;
  return a > o ? a : o;
}
FGX_HD constexpr int rollout_lds_bytes(int dof, int obs_dim) {
  return (int)sizeof(float) * kRolloutWaves * rollout_wave_floats(dof, obs_dim);
}
}  // namespace fgx
