// The episode-kernel selection table (csrc/fgx_select.h: select_episode_kernel) on the CPU, run by
// tests/test_host_select.py: a grid of synthetic DevCfg / SelectIn values and override settings, one
// line per case with the chosen kernel's name.  The output must equal tests/host/select_table.expected
// byte for byte; that file was recorded from the selection code as it stood before it moved into one
// function (hp_applies + episode_kernel_choice, the overrides set in the environment).  The CU count
// is an input (256: one k_episode round is 65536 envs), so no device is needed.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

// ---- the function under test
#include "../../fancy_gym_crowd_amd/csrc/fgx_select.h"

static int choose(const fgx::DevCfg& c, int mp, int info_level, bool per_env_plans, bool has_rew_scratch) {
  return fgx::select_episode_kernel(
      c, fgx::SelectIn::from_info_level(c, mp, info_level, per_env_plans, has_rew_scratch, 256),
      fgx::KernelOverrides::from_env());
}
// ---- the grid

using namespace fgx;

static const char* const kKernel[] = {"k_episode", "k_episode_jp", "k_episode_ws", "k_episode_jl", "k_episode_w2",
                                      "k_episode_pair", "k_episode_v2", "k_episode_v2h", "k_episode_hp"};
static const char* const kEnv[] = {"simple", "hole", "via"};
static const char* const kMp[] = {"none", "promp", "dmp", "prodmp", "given"};
static const char* const kCtrl[] = {"pd", "vel", "pos"};

struct Case {
  int env = ENV_SIMPLE, nl = 5, nb = 5, mp = MP_PROMP, ctrl = CTRL_PD, info = 0;
  long N = 256;
  int T = 100, max_steps = 200, rows = 202, stride = 8;   // (rows x stride: the basis table in LDS)
  int replan = 0, learn_tau = 0, learn_delay = 0, sched_state = 0, cond_desired = 0, valid_flags = 0;
  int rew_fct = REW_SIMPLE, per_env_plans = 0, rew_scratch = 1;
  const char* ek = nullptr;   // FGX_EPISODE_KERNEL, FGX_V2, FGX_HP (null: unset)
  const char* v2 = nullptr;
  const char* hp = nullptr;
};

static void put_env(const char* name, const char* v) {
  if (v) setenv(name, v, 1);
  else unsetenv(name);
}

static void emit(const Case& k) {
  DevCfg c = {};
  c.N = k.N;
  c.env = k.env;
  c.nl = k.nl;
  c.nb = k.nb;
  c.mp = k.mp == MP_GIVEN ? MP_PROMP : k.mp;   // (a caller-given plan on a handle built for ProMP)
  c.ctrl = k.ctrl;
  c.T = k.T;
  c.max_steps = k.max_steps;
  c.rows = k.rows;
  c.stride = k.stride;
  c.replan = k.replan;
  c.learn_tau = k.learn_tau;
  c.learn_delay = k.learn_delay;
  c.sched_state = k.sched_state;
  c.cond_desired = k.cond_desired;
  c.valid_flags = k.valid_flags;
  c.rew_fct = k.rew_fct;
  c.obs_dim = k.env == ENV_SIMPLE ? 3 * k.nl + 3 : (k.env == ENV_HOLE ? 3 * k.nl + 4 : 3 * k.nl + 5);
  c.full_dim = c.obs_dim;
  put_env("FGX_EPISODE_KERNEL", k.ek);
  put_env("FGX_V2", k.v2);
  put_env("FGX_HP", k.hp);
  const int id = choose(c, k.mp, k.info, k.per_env_plans != 0, k.rew_scratch != 0);
  std::printf("%s nl=%d nb=%d %s %s info=%d N=%ld T=%d ms=%d tab=%dx%d", kEnv[k.env], k.nl, k.nb, kMp[k.mp],
              kCtrl[k.ctrl], k.info, k.N, k.T, k.max_steps, k.rows, k.stride);
  if (k.replan) std::printf(" replan");
  if (k.learn_tau) std::printf(" learn_tau");
  if (k.learn_delay) std::printf(" learn_delay");
  if (k.sched_state) std::printf(" sched_state");
  if (k.cond_desired) std::printf(" cond_desired");
  if (k.valid_flags) std::printf(" valid_flags");
  if (k.rew_fct != REW_SIMPLE) std::printf(" rew_fct=%d", k.rew_fct);
  if (k.per_env_plans) std::printf(" per_env_plans");
  if (!k.rew_scratch) std::printf(" no_rew_scratch");
  if (k.ek) std::printf(" FGX_EPISODE_KERNEL=%s", k.ek);
  if (k.v2) std::printf(" FGX_V2=%s", k.v2);
  if (k.hp) std::printf(" FGX_HP=%s", k.hp);
  std::printf(" -> %s\n", id >= 0 && id < 9 ? kKernel[id] : "?");
}

// one round R of k_episode is 65536 envs: both sides of 2N <= R, 4N <= 3R, N > R, the tail rule
// 2 (N mod R) <= R (tail 32768 / 32769) and a zero tail; N % 256 zero and nonzero
static const long kSizes[] = {32, 256, 32768, 32769, 49152, 49153, 65536, 65537, 98304, 98305, 131072};

int main() {
  const int envs[] = {ENV_SIMPLE, ENV_HOLE, ENV_VIA};
  const int mps[] = {MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN};

  std::printf("# A: env x links x MP kind x controller x info level, no override; past one round for 5 links\n");
  for (int env : envs)
    for (int nl : {1, 2, 5, 8})
      for (int mp : mps)
        for (int ctrl : {CTRL_PD, CTRL_VEL})
          for (int info : {0, 1, 2})
            for (long N : {256L, 98304L}) {
              if (N != 256 && (nl != 5 || info != 0)) continue;
              Case k;
              k.env = env; k.nl = nl; k.mp = mp; k.ctrl = ctrl; k.info = info; k.N = N;
              emit(k);
            }

  std::printf("# B: the size rules (replanning enters SimpleReacher's only)\n");
  for (int env : envs)
    for (int nl : {2, 5})
      for (int replan : {0, 1})
        for (long N : kSizes) {
          if (env != ENV_SIMPLE && (nl != 5 || replan)) continue;
          Case k;
          k.env = env; k.nl = nl; k.replan = replan; k.N = N;
          emit(k);
        }

  std::printf("# C: each clause alone, from a base case of every kernel\n");
  Case bases[9];
  bases[0].info = 0;                                          // k_episode_jl
  bases[1].info = 2;                                          // k_episode_v2
  bases[2].N = 131072;                                        // k_episode_w2
  bases[3].env = ENV_HOLE;                                    // k_episode_hp
  bases[4].env = ENV_HOLE; bases[4].info = 1;                 // k_episode_hp, per-step arrays
  bases[5].env = ENV_HOLE; bases[5].info = 2;                 // k_episode_v2h
  bases[6].env = ENV_HOLE; bases[6].rew_fct = REW_VEL_ACC;    // k_episode_pair
  bases[7].env = ENV_VIA; bases[7].info = 1;                  // k_episode_v2h
  bases[8].env = ENV_HOLE; bases[8].hp = "1"; bases[8].info = 2;   // k_episode_hp forced onto the verbose-2 rows
  for (const Case& b : bases) {
    emit(b);
    Case k;
    k = b; k.nb = 7; emit(k);
    k = b; k.mp = MP_NONE; emit(k);
    k = b; k.mp = MP_GIVEN; emit(k);
    k = b; k.ctrl = CTRL_POS; emit(k);
    k = b; k.replan = 1; emit(k);
    k = b; k.learn_tau = 1; emit(k);
    k = b; k.learn_delay = 1; emit(k);
    k = b; k.sched_state = 1; emit(k);
    k = b; k.cond_desired = 1; emit(k);
    k = b; k.valid_flags = 1; emit(k);
    k = b; k.rew_fct = b.rew_fct == REW_SIMPLE ? REW_UNBOUNDED : REW_SIMPLE; emit(k);
    k = b; k.per_env_plans = 1; emit(k);
    k = b; k.rew_scratch = 0; emit(k);
    k = b; k.T = 256; emit(k);
    k = b; k.T = 257; emit(k);
    k = b; k.max_steps = 201; emit(k);
    k = b; k.N = b.N + 1; emit(k);
    // the 160 KiB LDS caps: 5 links, k_episode_v2h (HoleReacher) holds tables up to 41984 B,
    // k_episode_v2 up to 63488 B
    k = b; k.rows = 800; k.stride = 14; emit(k);   // 44800 B
    k = b; k.rows = 1000; k.stride = 16; emit(k);  // 64000 B
    k = b; k.rows = 656; k.stride = 16; emit(k);   // 41984 B
    k = b; k.rows = 992; k.stride = 16; emit(k);   // 63488 B
  }

  std::printf("# D: every override value alone, and the combinations whose precedence matters\n");
  struct Ov { const char* ek; const char* v2; const char* hp; };
  const Ov ovs[] = {
      {"classic", nullptr, nullptr}, {"jp", nullptr, nullptr}, {"ws", nullptr, nullptr}, {"jl", nullptr, nullptr},
      {"w2", nullptr, nullptr}, {"pair", nullptr, nullptr}, {"hp", nullptr, nullptr}, {"bogus", nullptr, nullptr},
      {"", nullptr, nullptr}, {nullptr, "0", nullptr}, {nullptr, "1", nullptr}, {nullptr, nullptr, "0"},
      {nullptr, nullptr, "1"}, {nullptr, nullptr, "2"},
      {"classic", nullptr, "1"}, {"hp", nullptr, "0"}, {"hp", nullptr, "1"}, {"bogus", nullptr, "1"},
      {nullptr, "0", "1"}, {"hp", "0", nullptr}, {"jl", "0", nullptr}, {"pair", "0", "0"}};
  for (const Ov& ov : ovs)
    for (int env : envs)
      for (int nl : {2, 5})
        for (int info : {0, 1, 2})
          for (long N : {256L, 131072L}) {
            if (nl == 2 && (env != ENV_SIMPLE || info == 1 || N != 256)) continue;
            if (N != 256 && info != 0) continue;
            Case k;
            k.env = env; k.nl = nl; k.info = info; k.N = N;
            k.ek = ov.ek; k.v2 = ov.v2; k.hp = ov.hp;
            emit(k);
          }

  std::printf("# E: forced kernels on the plans and controllers the shard kernels do not serve\n");
  for (const char* ek : {"classic", "w2", "jl", "jp", "ws"})
    for (int mp : {MP_PROMP, MP_GIVEN})
      for (int ctrl : {CTRL_PD, CTRL_VEL})
        for (long N : {256L, 131072L}) {
          Case k;
          k.mp = mp; k.ctrl = ctrl; k.N = N; k.ek = ek;
          emit(k);
        }
  return 0;
}
