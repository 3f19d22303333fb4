// fgx_wide.hip — the wide-basis plan GEMM (fgx_wide.h) and the info copy of its plans: one unit for
// every link count (the kernel's columns are flat, fgx_wide.h).
#include <algorithm>

#include "fgx_wide.h"

using namespace fgx;

const char* fgx_traj_wide_refusal(const DevCfg& c) {
  if (c.mp != MP_PROMP && c.mp != MP_PRODMP) return "ProMP / ProDMP only";
  if (c.replan || c.learn_tau || c.learn_delay || c.cond_desired) return "plans must all start on table row 0";
  if (c.T < 2) return "plan length T < 2 not supported";
  if (c.T > 32 * kWideWaves) return "plan length T > 256 not supported";
  if (c.nl < 1 || c.nl * kWideGE > kWideCols) return "n_links out of range";
  if (traj_wide_lds_bytes(c.T, c.nl) > 160 * 1024) return "plan length T x n_links exceeds the LDS staging region";
  return nullptr;
}

int fgx_launch_traj_wide(const DevCfg& c, const DevState& s, const float* params, float* dpos, float* dvel,
                         hipStream_t stream, std::string& err) {
  if (const char* why = fgx_traj_wide_refusal(c)) {
    err = std::string("k_traj_wide: ") + why;
    return -4;
  }
  const int vec = ((c.T * c.nl) & 3) == 0 && (((uintptr_t)dpos | (uintptr_t)dvel) & 15) == 0;
  const int64_t groups = (c.N + kWideGE - 1) / kWideGE;
  // one workgroup per CU (its LDS), each walking groups
  const dim3 grid((unsigned)std::min<int64_t>(groups, device_cus())), block(kWideThreads);
  const size_t lds = traj_wide_lds_bytes(c.T, c.nl);
  return pick<MP_PROMP, MP_PRODMP>(c.mp, -1, "k_traj_wide: ProMP / ProDMP only", err, [&](auto MP) {
    return launch("k_traj_wide", k_traj_wide<MP>, grid, block, lds, stream, err, c, s, params, dpos, dvel, vec);
  });
}

int fgx_launch_plan_info(const DevCfg& c, const float* dpos, const float* dvel, float* info_pos, float* info_vel,
                         hipStream_t stream, std::string& err) {
  const int run = c.T * c.nl;
  const dim3 grid((unsigned)((c.N + 63) / 64), (unsigned)((run + 63) / 64)), block(256);
  return launch("k_plan_info", k_plan_info, grid, block, 0, stream, err, c.N, run, dpos, dvel, info_pos, info_vel);
}
