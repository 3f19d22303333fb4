// fgx_ep_nl.h — what a handle of FGX_NL links launches: the NlOps table (fgx_launch.h) of one link
// count (include/fgx.h n_links 1..8; the reference env takes any n_links, base_reacher.py:17-39, and
// bb_env_constructor forwards env kwargs, envs/registry.py:280-281).  Included once by each
// fgx_ep_nl<n>.hip, which defines FGX_NL, so that the counts compile in parallel.  Reset, step-based
// step and rollout, trajectories and the learned-phase plans are the same templates at every count.  The
// registered counts 2 and 5 differ in three places, all below (kRegistered<NL>):
//   * NB: they also hold the NB = 5 forms of k_traj_valu / k_traj_env (kNB5<NL>; the others: the
//     generic basis count NB = 0 only, any n_basis <= 12);
//   * traj: they try k_traj_mfma first;
//   * episode: their episode kernels live in the env-kind units (fgx_ep_<env>[_gen].hip, fgx_ep_jl.hip,
//     fgx_ep_hp.hip) and this unit only routes to them; the others hold the logging k_episode here
//     (fgx_dispatch.h LOG_ONLY: it serves every info level and the validity checks).
// Sums over the joints follow numpy's order at every count (np_sum, fgx_device.h: the pairwise tree at 8).
#pragma once
#include "fgx_dispatch.h"
#include "fgx_learned.h"
#include "fgx_nl_pick.h"
#include "fgx_rollout.h"
#include "fgx_step.h"
#include "fgx_traj_run.h"

#define FGX_NL_CAT2(a, b) a##b
#define FGX_NL_CAT(a, b) FGX_NL_CAT2(a, b)

// k_rollout_seq of this link count: a unit of its own (fgx_seq_nl<n>.hip -> fgx_seq_nl.h)
int FGX_NL_CAT(fgx_launch_rollout_seq_, FGX_NL)(const fgx::DevCfg& c, const fgx::DevState& s, const float* params,
                                                int n_seg, int n_cand, const fgx::Outputs& o, int32_t* segments,
                                                double* seg_ret, int32_t* seg_len, hipStream_t stream,
                                                std::string& err);

namespace {
using namespace fgx;
// (kRegistered<NL>, kNB5<NL> and pick_mp_nb<NL>: fgx_nl_pick.h)

// (templates on the count, so that `if constexpr` leaves the branch not taken uninstantiated)
template <int NL>
int nl_episode(const DevCfg& c, const DevState& s, int mp, int kernel, const float* params, const float* dpos,
               const float* dvel, const Outputs& o, hipStream_t stream, std::string& err) {
  if constexpr (kRegistered<NL>) {
    // HoleReacher up to info level 1: the producer / consumer pipeline (fgx_hp.h)
    if (kernel == EK_HP) return fgx_launch_episode_hp(c, s, mp, params, o, stream, err);
    const bool gen = mp != MP_GIVEN && c.nb != 5;   // generic basis-count instantiations
    switch (c.env) {
      case ENV_SIMPLE:
        return (gen ? fgx_launch_episode_simple_gen : fgx_launch_episode_simple)(c, s, mp, kernel, params, dpos, dvel, o,
                                                                               stream, err);
      case ENV_HOLE:
        return (gen ? fgx_launch_episode_hole_gen : fgx_launch_episode_hole)(c, s, mp, kernel, params, dpos, dvel, o,
                                                                           stream, err);
      case ENV_VIA:
        return (gen ? fgx_launch_episode_via_gen : fgx_launch_episode_via)(c, s, mp, kernel, params, dpos, dvel, o,
                                                                         stream, err);
    }
  } else {
    return pick<ENV_SIMPLE, ENV_HOLE, ENV_VIA>(c.env, -1, "bad env kind", err, [&](auto ENV) {
      return launch_episode_env<ENV, 0, NL>(c, s, mp, kernel, params, dpos, dvel, o, stream, err);
    });
  }
  err = "bad env kind";
  return -1;
}

template <int NL>
int nl_reset(const DevCfg& c, const DevState& s, const uint64_t* seeds, const uint8_t* mask, int rs_mode, float* obs,
             hipStream_t stream, std::string& err) {
  const int threads = 256;
  return launch("k_reset", k_reset<NL>, dim3((unsigned)((c.N + threads - 1) / threads)), dim3(threads), 0, stream, err,
                c, s, seeds, mask, rs_mode, obs);
}

template <int NL>
int nl_step_raw(const DevCfg& c, const DevState& s, const float* act, float* obs, double* rew, uint8_t* term,
                uint8_t* trunc, float* final_obs, int autoreset, hipStream_t stream, std::string& err) {
  const dim3 grid((unsigned)((c.N + kStepRawBlock - 1) / kStepRawBlock)), block(kStepRawBlock);
  // LDS rows of the workgroup's action / observation slices (k_step_raw)
  const int so = step_raw_stride(c.obs_dim), sa = step_raw_stride(NL);
  const size_t lds = sizeof(float) * kStepRawBlock * ((so > sa ? so : sa) + (final_obs ? so : 0));
  return pick<ENV_SIMPLE, ENV_HOLE, ENV_VIA>(c.env, -1, "bad env kind", err, [&](auto ENV) {
    return launch("k_step_raw", k_step_raw<ENV, NL>, grid, block, lds, stream, err, c, s, act, obs, rew, term, trunc,
                  final_obs, autoreset);
  });
}

template <int NL>
int nl_rollout_raw(const DevCfg& c, const DevState& s, const float* act, int horizon, int n_cand, double* ret,
                   int32_t* len, uint8_t* term, uint8_t* trunc, float* obs, double* rew, int commit, hipStream_t stream,
                   std::string& err) {
  const int64_t blocks = (int64_t)n_cand * ((c.N + kRolloutBlock - 1) / kRolloutBlock);
  if (blocks > 0x7fffffff) {
    err = "k_rollout_raw: n_cand * ceil(n_envs / 256) workgroups exceed the grid limit";
    return -4;
  }
  // LDS regions of the four waves' action chunks / observation rows (k_rollout_raw, fgx_rollout_lds.h)
  const size_t lds = (size_t)rollout_lds_bytes(NL, obs ? c.obs_dim : 0);
  return pick<ENV_SIMPLE, ENV_HOLE, ENV_VIA>(c.env, -1, "bad env kind", err, [&](auto ENV) {
    return launch("k_rollout_raw", k_rollout_raw<ENV, NL>, dim3((unsigned)blocks), dim3(kRolloutBlock), lds, stream, err,
                  c, s, act, horizon, n_cand, ret, len, term, trunc, obs, rew, commit);
  });
}

// k_rollout_bb: one kernel family and one occupancy form, no selection.  THE RULE: the uncapped form
// at every C * N; the two-waves form (amdgpu_waves_per_eu(2)) measured the same within the
// alternation's spread at C * N = 65536 and 2^20 (ProMP LongSimpleReacher: 64.6 / 64.5 us and
// 645.4 / 645.4 us, profiles/rollout_bb.jsonl) because the rollout body already fits 256 registers.
template <int NL>
int nl_rollout_bb(const DevCfg& c, const DevState& s, const float* params, int n_cand, const Outputs& o,
                  hipStream_t stream, std::string& err) {
  const int64_t blocks = (int64_t)n_cand * ((c.N + 255) / 256);
  if (blocks > 0x7fffffff) {
    err = "k_rollout_bb: n_cand * ceil(n_envs / 256) workgroups exceed the grid limit";
    return -4;
  }
  const size_t lds = (size_t)c.rows * c.stride * sizeof(float);
  return pick<ENV_SIMPLE, ENV_HOLE, ENV_VIA>(c.env, -1, "bad env kind", err, [&](auto ENV) {
    return pick<CTRL_PD, CTRL_VEL, CTRL_POS>(c.ctrl, -1, "bad ctrl_kind", err, [&](auto CTRL) {
      return pick_mp_nb<NL>(c, "fgx_rollout_bb needs a movement primitive", err, [&](auto MP, auto NB) {
        if constexpr (NB != 0) {
          if (c.stride != Traj<MP, 1, NB>::KS) {
            err = "basis table stride does not match the compiled layout";
            return -1;
          }
        }
        return launch("k_rollout_bb launch", k_rollout_bb<ENV, MP, CTRL, NL, NB>, dim3((unsigned)blocks), dim3(256), lds,
                      stream, err, c, s, params, o);
      });
    });
  });
}

// k_traj_mfma (2 / 5 links), else k_traj_run, else k_traj_valu: the first that takes the plan
template <int NL>
int nl_traj(const DevCfg& c, const DevState& s, const float* params, float* dpos, float* dvel, hipStream_t stream,
            std::string& err) {
  return pick_mp_nb<NL>(c, "step-based handle has no trajectory generator", err, [&](auto MP, auto NB) {
    if constexpr (kRegistered<NL>)
      if (const int rm = launch_traj_mfma<NL>(c, s, params, dpos, dvel, stream, err); rm != 1) return rm;
    if (const int rr = launch_traj_run<NL>(c, s, params, dpos, dvel, stream, err); rr != 1) return rr;
    const int threads = 256;
    return launch("k_traj_valu", k_traj_valu<MP, NL, NB>, dim3((unsigned)((c.N + threads - 1) / threads)), dim3(threads),
                  0, stream, err, c, s, params, dpos, dvel);
  });
}

template <int NL>
int nl_traj_env(const DevCfg& c, const DevState& s, const float* params, float* env_tab, float* dpos, float* dvel,
                int32_t* plan_len, float* info_pos, float* info_vel, hipStream_t stream, std::string& err) {
  return pick_mp_nb<NL>(c, "learned phase parameters need a movement primitive", err, [&](auto MP, auto NB) {
    const int threads = 256;
    return launch("k_traj_env", k_traj_env<MP, NL, NB>, dim3((unsigned)((c.N + threads - 1) / threads)), dim3(threads), 0,
                  stream, err, c, s, params, env_tab, dpos, dvel, plan_len, info_pos, info_vel);
  });
}
}  // namespace

const fgx::NlOps* FGX_NL_CAT(fgx_nl_ops_, FGX_NL)() {
  static const fgx::NlOps ops = {nl_episode<FGX_NL>, nl_reset<FGX_NL>, nl_step_raw<FGX_NL>, nl_traj<FGX_NL>,
                                 nl_traj_env<FGX_NL>, nl_rollout_raw<FGX_NL>, nl_rollout_bb<FGX_NL>,
                                 FGX_NL_CAT(fgx_launch_rollout_seq_, FGX_NL)};
  return &ops;
}
