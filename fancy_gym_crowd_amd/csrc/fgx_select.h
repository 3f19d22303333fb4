// fgx_select.h — which episode kernel serves a black-box step: the one place that decides.
//
// select_episode_kernel is a pure host function of the handle's configuration, what the step asks
// for (SelectIn) and the override variables (KernelOverrides).  fgx_step / fgx_step_traj call it once
// per step and pass the id down to the translation unit that holds the kernel (fgx_dispatch.h:
// launch_episode_nl switches on it); fgx_episode_kernel reports the same function's answer.
#pragma once
#include <cstdlib>
#include <cstring>

#include "fgx_v2.h"

namespace fgx {

// Episode kernels: k_episode (fgx_kernels.h, one env per lane, every case), k_episode_jl (fgx_jl.h,
// one lane per env x joint), k_episode_jp (fgx_jp.h, one wave per joint) and k_episode_ws
// (fgx_ws.h, trajectory-producer / dynamics-consumer wave pairs).  The last three serve
// SimpleReacher + PD over the shared basis tables with static replanning schedules,
// max_episode_steps <= 200 and no per-step info, bit-identically to k_episode (tests/test_gpu_jl.py,
// test_gpu_jp.py, test_gpu_ws.py).  k_episode_w2 / k_episode_pair (fgx_kernels.h), k_episode_v2
// (fgx_v2.h), k_episode_v2h (fgx_kernels.h) and k_episode_hp (fgx_hp.h) are described at their rules
// below.  The ids are fgx_episode_kernel's (include/fgx.h).
enum : int {
  EK_CLASSIC = 0, EK_JP = 1, EK_WS = 2, EK_JL = 3, EK_CLASSIC_W2 = 4, EK_PAIR = 5, EK_V2 = 6, EK_V2H = 7, EK_HP = 8
};

// The override variables (A/B benchmarks, tests), read at every call: tests change them inside one
// process.  A forced kernel wins wherever it applies:
//   FGX_EPISODE_KERNEL=classic|jp|ws|jl|w2|pair|hp   any value but "hp" (an unknown one too) keeps
//                                                    k_episode_hp out; an empty value counts as unset
//   FGX_V2=0   keeps the logging k_episode where k_episode_v2 / _v2h (and k_episode_hp's INFO form) would run
//   FGX_HP=0   never k_episode_hp;  FGX_HP=1 also gives it the verbose-2 rows
//   FGX_WIDE=1 a handle created under it plans with k_traj_wide wherever that kernel applies (fgx_api.hip
//              wide_eligible), also at n_basis <= 12: the A/B and equivalence switch of the wide path
struct KernelOverrides {
  enum Kernel { K_UNSET, K_CLASSIC, K_JP, K_WS, K_JL, K_W2, K_PAIR, K_HP, K_UNKNOWN };
  enum Switch { S_UNSET, S_OFF, S_FORCE };
  Kernel kernel = K_UNSET;
  Switch v2 = S_UNSET;   // S_OFF only
  Switch hp = S_UNSET;
  bool wide = false;     // FGX_WIDE=1: read by fgx_create, not by select_episode_kernel

  static KernelOverrides from_env() {
    KernelOverrides ov;
    if (const char* v = std::getenv("FGX_WIDE")) ov.wide = std::strcmp(v, "1") == 0;
    if (const char* v = std::getenv("FGX_EPISODE_KERNEL")) {
      static const char* const names[] = {"classic", "jp", "ws", "jl", "w2", "pair", "hp"};
      if (*v) ov.kernel = K_UNKNOWN;
      for (int i = 0; i < 7; ++i)
        if (std::strcmp(v, names[i]) == 0) ov.kernel = (Kernel)(K_CLASSIC + i);
    }
    if (const char* v = std::getenv("FGX_V2"))
      if (std::strcmp(v, "0") == 0) ov.v2 = S_OFF;
    if (const char* v = std::getenv("FGX_HP"))
      ov.hp = std::strcmp(v, "0") == 0 ? S_OFF : std::strcmp(v, "1") == 0 ? S_FORCE : S_UNSET;
    return ov;
  }
};

// some per-step array of the step's info is written
inline bool step_rows(const Outputs& o) {
  return o.positions || o.step_actions || o.step_obs || o.step_rewards || o.is_collided || o.end_effector ||
         o.reward_dist;
}
// any per-step output, or the validity checks (c.valid_flags, which only the logging instantiations
// run): the logging instantiations
inline bool episode_logs(const DevCfg& c, const Outputs& o) { return step_rows(o) || c.valid_flags != 0; }

// What the decision reads besides DevCfg.
struct SelectIn {
  int mp;               // the effective MP kind: MP_GIVEN for caller-given and per-env (learned) plans
  bool log;             // a logging instantiation is needed (episode_logs)
  bool heavy;           // the verbose-2 rows: planned positions / velocities, step observations
  bool per_env_plans;   // per-env plan lengths (learned tau / delay)
  bool has_rew_scratch; // the handle's [T][N] step-reward scratch exists (DevState::rew)
  int cus;              // the device's CU count (device_cus())

  // the launch path: from the step's output pointers
  static SelectIn from_outputs(const DevCfg& c, int mp, const Outputs& o, bool per_env_plans, bool has_rew_scratch,
                               int cus) {
    return make(c, mp, step_rows(o), o.positions || o.step_obs, per_env_plans, has_rew_scratch, cus);
  }
  // fgx_episode_kernel: from the info level (include/fgx.h: 1 = the light per-step arrays, 2 = all)
  static SelectIn from_info_level(const DevCfg& c, int mp, int info_level, bool per_env_plans, bool has_rew_scratch,
                                  int cus) {
    return make(c, mp, info_level >= 1, info_level >= 2, per_env_plans, has_rew_scratch, cus);
  }

 private:
  static SelectIn make(const DevCfg& c, int mp, bool rows, bool heavy_rows, bool per_env_plans, bool has_rew_scratch,
                       int cus) {
    return SelectIn{mp, rows || c.valid_flags != 0, heavy_rows, per_env_plans, has_rew_scratch, cus};
  }
};

// envs of one k_episode round: one 64-lane wave per SIMD
inline int64_t round_envs(int cus) { return (int64_t)cus * 4 * 64; }

// k_episode and its variants (fgx_kernels.h), for whatever the specialised kernels do not take
inline int classic_choice(const DevCfg& c, const SelectIn& in, const KernelOverrides& ov) {
  const bool keep_classic = ov.kernel == KernelOverrides::K_CLASSIC;
  // k_episode_v2h: the per-step info rows of the direct envs (HoleReacher, ViaPointReacher) stored by
  // a partner wave per SIMD; whole 256-env workgroups only.  FGX_V2=0 (or FGX_EPISODE_KERNEL=classic)
  // keeps the logging k_episode
  if (in.log && !keep_classic && ov.v2 != KernelOverrides::S_OFF && c.env != ENV_SIMPLE && c.N % 256 == 0 &&
      (c.nl == 2 || c.nl == 5) && v2h_lds_bytes(c.mp, c.rows, c.stride, c.nl, c.full_dim) <= 160 * 1024)
    return EK_V2H;
  if (in.log || c.nl != 5 || keep_classic) return EK_CLASSIC;
  // k_episode_pair: 5-link HoleReacher without per-step info (two lanes per env, fgx_kernels.h) while
  // its 2N lanes fit one wave per SIMD (N <= 32768 on 256 CUs): each lane issues 15% fewer VALU
  // instructions than k_episode's (16384 / 32768 envs: 487 / 493 vs 517 / 525 us).  Past that the
  // pairs' second wave per SIMD does not pay for the duplicated plan / controller / dynamics work
  // (65536: 648 vs 530 us; profiles/r03_pair_scan.jsonl).  FGX_EPISODE_KERNEL=pair forces it
  if (c.env == ENV_HOLE)
    return ov.kernel == KernelOverrides::K_PAIR || 2 * c.N <= round_envs(in.cus) ? EK_PAIR : EK_CLASSIC;
  // k_episode_w2: 5-link SimpleReacher without per-step info past one k_episode round (two resident
  // waves per SIMD, profiles/r02_w2_ab.jsonl).  FGX_EPISODE_KERNEL=w2 forces it
  if (c.env == ENV_SIMPLE)
    return ov.kernel == KernelOverrides::K_W2 || c.N > round_envs(in.cus) ? EK_CLASSIC_W2 : EK_CLASSIC;
  return EK_CLASSIC;
}

inline int select_episode_kernel(const DevCfg& c, const SelectIn& in, const KernelOverrides& ov) {
  using O = KernelOverrides;
  // what every specialised kernel asks of the plan: generated from the shared basis tables (no
  // caller-given or per-env plans, no learned tau / delay), a static replanning schedule, and an
  // episode short enough for the in-register pairwise return
  const bool shared_static_plan = (in.mp == MP_PROMP || in.mp == MP_DMP || in.mp == MP_PRODMP) && !in.per_env_plans &&
                                  !c.learn_tau && !c.learn_delay && !c.sched_state && c.T <= 256 && c.max_steps <= 200;

  // k_episode_hp (fgx_hp.h): HoleReacher with the simple reward, 5 links, 5 basis functions, up to
  // info level 1, as a producer / consumer pipeline; its candidate final states live in the handle's
  // reward scratch.  With per-step arrays it runs its INFO instantiation (FGX_V2=0 keeps the logging
  // k_episode there).  On the verbose-2 rows k_episode_v2h stays faster (65536 envs: 1026 vs 1637 us,
  // profiles/r05_s9_jlhelper_traj_hpinfo.jsonl), so k_episode_hp takes them only when forced (FGX_HP=1)
  if (ov.hp != O::S_OFF && (!in.heavy || ov.hp == O::S_FORCE) && (ov.kernel == O::K_UNSET || ov.kernel == O::K_HP) &&
      !(in.log && ov.v2 == O::S_OFF) && shared_static_plan && c.env == ENV_HOLE && c.rew_fct == REW_SIMPLE &&
      c.nl == 5 && c.nb == 5 && !c.cond_desired && c.valid_flags == 0 && in.has_rew_scratch)
    return EK_HP;

  const bool simple_pd = shared_static_plan && c.env == ENV_SIMPLE && c.ctrl == CTRL_PD && (c.nl == 2 || c.nl == 5);
  if (!simple_pd) return classic_choice(c, in, ov);

  // k_episode_v2 (fgx_v2.h): the per-step info arrays of SimpleReacher + PD (info_level >= 1, the
  // reference's verbose-2 default) with the observation's trigonometry on a second wave of each SIMD;
  // FGX_V2=0 (or FGX_EPISODE_KERNEL=classic) keeps the logging k_episode, which also runs the
  // validity checks
  if (in.log) {
    if (ov.v2 != O::S_OFF && ov.kernel != O::K_CLASSIC && c.valid_flags == 0 &&
        v2_lds_bytes(c.rows, c.stride, c.nl) <= 160 * 1024)
      return EK_V2;
    return classic_choice(c, in, ov);
  }

  // No per-step info: the shard kernels.  k_episode_jp and k_episode_ws stay selectable:
  // FGX_EPISODE_KERNEL=classic|w2|jp|ws|jl forces a kernel wherever it applies
  switch (ov.kernel) {
    case O::K_CLASSIC:
    case O::K_W2: return classic_choice(c, in, ov);
    case O::K_JP: return EK_JP;
    case O::K_WS: return EK_WS;
    case O::K_JL: return EK_JL;
    default: break;
  }
  // Which one runs follows the measured table profiles/r02_kernel_scan_all.jsonl (every kernel forced
  // over envs per GPU x MP kind x links on one MI355X, tools/scan_all.sh):
  //  * k_episode holds one wave (64 envs) per SIMD: a near-fixed ~73-105 us (5 links) up to one full
  //    round of 65536 envs, where its 5 independent joint chains per lane keep the lone wave busy;
  //  * k_episode_jl puts 5x the lanes to work below that (8192 envs: 26 us vs 41 us k_episode_jp and
  //    61 us k_episode, ProMP 5 links) and wins at every size for 2 links (the 2-link k_episode is a
  //    short-chain lone wave too), replanning included;
  //  * past one round whose last round is at most half full (5 links), k_episode_jl again (98304 envs:
  //    112 us vs 127 us k_episode, profiles/r02_jl_scan.jsonl; it took k_episode_jp's place there once
  //    its exchange rows stopped conflicting on LDS banks).
  const int64_t R = round_envs(in.cus), tail = c.N % R;
  if (c.nl == 2) return EK_JL;
  if (4 * c.N <= 3 * R) return EK_JL;
  if (!c.replan && c.N > R && tail != 0 && 2 * tail <= R) return EK_JL;
  return classic_choice(c, in, ov);
}

}  // namespace fgx
