// fgx_launch.h — how every unit gets from run-time kinds to a launched kernel, and what the units
// offer each other.  The rule a kernel family follows: pick<...> each run-time kind into a template
// argument (nested, `if constexpr` on the tags for what the unit does not instantiate), then launch(...)
// (fgx_device.h) with the family's grid, block and LDS size.  The declarations below are functions
// only, so the C ABI unit (fgx_api.hip) reaches every kernel family without seeing a kernel template.
// All return 0 or an FGX_E_* code (-1 bad kind / no MP, -2 HIP error, -4 not instantiated), message in err.
#pragma once
#include <string>
#include <type_traits>

#include "fgx_device.h"

namespace fgx {
// Calls f(std::integral_constant<int, V>{}) for the first listed V that equals v and returns its
// result; no V equals v: f is not called, err = miss, returns miss_code.  (A bool: pick<0, 1>.)
template <int... Vs, class F>
int pick(int v, int miss_code, const char* miss, std::string& err, F&& f) {
  int rc = miss_code;
  bool hit = false;
  ((v == Vs && !hit ? (hit = true, rc = f(std::integral_constant<int, Vs>{}), 0) : 0), ...);
  if (!hit) err = miss;
  return rc;
}
}  // namespace fgx

// k_episode and its variants per env kind (fgx_ep_<env>.hip: NB = 5; fgx_ep_<env>_gen.hip: NB = 0), 2 / 5
// links; kernel: the EK_* id select_episode_kernel chose (fgx_select.h)
#define FGX_DECLARE_LAUNCH(NAME)                                                                             \
  int NAME(const fgx::DevCfg& c, const fgx::DevState& s, int mp, int kernel, const float* params,            \
           const float* dpos, const float* dvel, const fgx::Outputs& o, hipStream_t stream, std::string& err);
FGX_DECLARE_LAUNCH(fgx_launch_episode_simple)
FGX_DECLARE_LAUNCH(fgx_launch_episode_hole)
FGX_DECLARE_LAUNCH(fgx_launch_episode_via)
FGX_DECLARE_LAUNCH(fgx_launch_episode_simple_gen)
FGX_DECLARE_LAUNCH(fgx_launch_episode_hole_gen)
FGX_DECLARE_LAUNCH(fgx_launch_episode_via_gen)
#undef FGX_DECLARE_LAUNCH
// k_episode_jl instantiations (fgx_ep_jl.hip): nbs = the compiled basis count (5, or 0 = generic)
int fgx_launch_episode_jl(const fgx::DevCfg& c, const fgx::DevState& s, int mp, int nbs, const float* params,
                          const fgx::Outputs& o, hipStream_t stream, std::string& err);
// k_episode_hp instantiations (fgx_ep_hp.hip)
int fgx_launch_episode_hp(const fgx::DevCfg& c, const fgx::DevState& s, int mp, const float* params,
                          const fgx::Outputs& o, hipStream_t stream, std::string& err);

// k_traj_wide (fgx_wide.hip): the plans of a wide handle (n_basis above the episode kernels' register
// slots, or FGX_WIDE=1) as an f32 MFMA GEMM over the shared table, every link count from one unit.
// fgx_traj_wide_refusal: null, or why k_traj_wide cannot take the configuration (fgx_create refuses
// it with that text).  fgx_launch_plan_info: the plans [N, T, dof] into info's [T, dof, N] arrays.
const char* fgx_traj_wide_refusal(const fgx::DevCfg& c);
int fgx_launch_traj_wide(const fgx::DevCfg& c, const fgx::DevState& s, const float* params, float* dpos, float* dvel,
                         hipStream_t stream, std::string& err);
int fgx_launch_plan_info(const fgx::DevCfg& c, const float* dpos, const float* dvel, float* info_pos, float* info_vel,
                         hipStream_t stream, std::string& err);

namespace fgx {
// What a handle launches, per link count (include/fgx.h: n_links 1..8; base_reacher.py:17-39 takes any
// count and bb_env_constructor forwards env kwargs, envs/registry.py:280-281): one translation unit
// per count (fgx_ep_nl<n>.hip -> fgx_ep_nl.h) fills this table, and fgx_api.hip launches through it only.
struct NlOps {
  int (*episode)(const DevCfg& c, const DevState& s, int mp, int kernel, const float* params, const float* dpos,
                 const float* dvel, const Outputs& o, hipStream_t stream, std::string& err);
  int (*reset)(const DevCfg& c, const DevState& s, const uint64_t* seeds, const uint8_t* mask, int rs_mode, float* obs,
               hipStream_t stream, std::string& err);
  int (*step_raw)(const DevCfg& c, const DevState& s, const float* act, float* obs, double* rew, uint8_t* term,
                  uint8_t* trunc, float* final_obs, int autoreset, hipStream_t stream, std::string& err);
  int (*traj)(const DevCfg& c, const DevState& s, const float* params, float* dpos, float* dvel, hipStream_t stream,
              std::string& err);
  int (*traj_env)(const DevCfg& c, const DevState& s, const float* params, float* env_tab, float* dpos, float* dvel,
                  int32_t* plan_len, float* info_pos, float* info_vel, hipStream_t stream, std::string& err);
  // k_rollout_raw: horizon steps of n_cand action sequences per env (fgx_rollout_raw, include/fgx.h)
  int (*rollout_raw)(const DevCfg& c, const DevState& s, const float* act, int horizon, int n_cand, double* ret,
                     int32_t* len, uint8_t* term, uint8_t* trunc, float* obs, double* rew, int commit,
                     hipStream_t stream, std::string& err);
  // k_rollout_bb: the black-box step of n_cand parameter rows per env, the handle left as it is
  // (fgx_rollout_bb, include/fgx.h); s.rew: the caller's workspace, o: the candidate-row outputs
  int (*rollout_bb)(const DevCfg& c, const DevState& s, const float* params, int n_cand, const Outputs& o,
                    hipStream_t stream, std::string& err);
  // k_rollout_seq: up to n_seg successive black-box steps of n_cand parameter sequences per env
  // (fgx_rollout_bb_seq, include/fgx.h); s.rew and o as for rollout_bb, o.tlen / o.ret: the sums
  int (*rollout_seq)(const DevCfg& c, const DevState& s, const float* params, int n_seg, int n_cand, const Outputs& o,
                     int32_t* segments, double* seg_ret, int32_t* seg_len, hipStream_t stream, std::string& err);
};
}  // namespace fgx
const fgx::NlOps* fgx_nl_ops_1();
const fgx::NlOps* fgx_nl_ops_2();
const fgx::NlOps* fgx_nl_ops_3();
const fgx::NlOps* fgx_nl_ops_4();
const fgx::NlOps* fgx_nl_ops_5();
const fgx::NlOps* fgx_nl_ops_6();
const fgx::NlOps* fgx_nl_ops_7();
const fgx::NlOps* fgx_nl_ops_8();
