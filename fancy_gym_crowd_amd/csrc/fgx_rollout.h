// fgx_rollout.h — k_rollout_raw: H step-based env.steps of C open-loop action sequences per env in
// one launch (fgx_rollout_raw, include/fgx.h; the reference loop: base_reacher.py:98-119 called H
// times from each env's current state).  The step-based counterpart of the fused episode: the env
// is loaded once, stepped in registers by the same substep<ENV, true, NL> call as k_step_raw, and
// stored only under `commit`.  Own header: only the per-link-count units (fgx_ep_nl.h) instantiate it.
#pragma once
#include "fgx_rollout_lds.h"
#include "fgx_step.h"

namespace fgx {

static_assert(rollout_stride(5) == step_raw_stride(5) && rollout_stride(8) == step_raw_stride(8),
              "the rollout stages its rows as k_step_raw does");

// One thread per (env, candidate).  A workgroup covers 256 consecutive envs of one candidate (grid =
// C · ceil(N / 256)): the state arrays [rows][N] load coalesced by e, the outputs [C, N] store
// coalesced by c·N + e, and the workgroup's action slice of one step, actions[h, c, e0 .. e0 + 256, :],
// is one contiguous run.  Each wave owns its 64 envs of that run and stages their rows through its
// own LDS region (fgx_rollout_lds.h) a chunk of steps at a time: every HBM wave-instruction reads
// 64 consecutive floats, the lanes read their rows at an odd stride, and the next chunk's loads
// stay in flight in registers while the current chunk's steps run.  Nothing is shared between the
// waves, so the kernel has no workgroup barrier and a wave leaves the step loop as soon as none of
// its lanes is alive (lanes stop at different lengths L: `alive`).  Per-step rewards [H, C, N] are
// direct stores, 64 consecutive doubles per wave-instruction, +0.0 from step L on; the final
// observation rows leave through the wave's LDS region as k_step_raw's do.
template <int ENV, int NL>
__global__ __launch_bounds__(kRolloutBlock) void k_rollout_raw(DevCfg c, DevState s, const float* __restrict__ act,
                                                               int H, int C, double* ret, int32_t* len, uint8_t* term,
                                                               uint8_t* trunc, float* obs, double* rew, int commit) {
  constexpr int K = rollout_chunk(NL), sa = rollout_stride(NL);
  extern __shared__ float lds_rollout[];
  const int od = c.obs_dim, so = rollout_stride(od);
  const int64_t N = c.N;
  const int nblk = (int)((N + kRolloutBlock - 1) / kRolloutBlock);
  const int cand = (int)(blockIdx.x / nblk);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)(blockIdx.x % nblk) * kRolloutBlock + 64 * wave;   // the wave's first env
  if (w0 >= N || cand >= C) return;   // (wave-uniform; the tail workgroup's empty waves)
  const int nw = (int)((N - w0) < 64 ? (N - w0) : 64);   // envs of this wave
  const int64_t e = w0 + lane;
  const bool live = lane < nw;
  float* lw = lds_rollout + wave * rollout_wave_floats(NL, obs ? od : 0);

  // the wave's rows of steps h0 .. h0 + K: element i of a step's run of nw · NL floats sits in lane i % 64
  float pf[K * NL];
  auto fetch = [&](int h0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float* ag = act + (((int64_t)(h0 + k) * C + cand) * N + w0) * NL;
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane + 64 * j;
        pf[k * NL + j] = (h0 + k < H && i < nw * NL) ? ag[i] : 0.f;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane + 64 * j;   // (rows nw .. 63 take the zeros)
        lw[(k * 64 + i / NL) * sa + i % NL] = pf[k * NL + j];
      }
  };

  Env<NL> v;
  if (live) load_env(c, s, e, v, ENV != ENV_SIMPLE);
  fetch(0);
  bool alive = live, te = false, tr = false;
  int L = 0, h = 0;
  double R = 0.0;
  while (h < H && __ballot(alive) != 0) {
    wave_lds_sync();   // the previous chunk's rows are read
    stage();
    wave_lds_sync();
    if (h + K < H) fetch(h + K);   // in flight during this chunk's steps
    const int hc = h + K < H ? h + K : H;
#pragma nounroll
    for (int k = 0; h < hc && __ballot(alive) != 0; ++k, ++h) {
      double r_h = 0.0;
      if (alive) {
        float a32[NL];
        double a[NL];
#pragma unroll
        for (int d = 0; d < NL; ++d) { a32[d] = lw[(k * 64 + lane) * sa + d]; a[d] = (double)a32[d]; }
        const StepOut r = substep<ENV, true, NL>(c, v, a, a32, true);
        te = (ENV != ENV_SIMPLE) && r.coll;
        tr = v.steps >= c.max_steps;
        r_h = r.reward;
        R = h == 0 ? r_h : R + r_h;   // ((r_0 + r_1) + r_2) + ...
        L = h + 1;
        alive = !(te || tr);
      }
      if (rew && live) rew[((int64_t)h * C + cand) * N + e] = r_h;
    }
  }
  if (rew && live)
    for (; h < H; ++h) rew[((int64_t)h * C + cand) * N + e] = 0.0;
  if (live) {
    const int64_t o = (int64_t)cand * N + e;
    ret[o] = R;
    len[o] = L;
    term[o] = te;
    trunc[o] = tr;
    if (commit) store_env(c, s, e, v, ENV != ENV_SIMPLE);
  }
  if (obs) {
    wave_lds_sync();   // the last chunk's rows are read: the region takes the observations
    if (live) emit_obs(c, v, false, lw + lane * so, nullptr);
    wave_lds_sync();
    float* og = obs + ((int64_t)cand * N + w0) * od;
    for (int i = lane; i < nw * od; i += 64) og[i] = lw[(i / od) * so + i % od];
  }
}

}  // namespace fgx
