// fgx_dispatch.h — template dispatch of the episode kernel.  One translation unit per env kind
// and basis specialisation for 2 / 5 links (fgx_ep_<env>.hip: NB = 5, the registered configs;
// fgx_ep_<env>_gen.hip: NB = 0, the generic runtime basis count) and one per further link count
// (fgx_ep_nl.h, the logging kernel only), so that the build compiles them in parallel.  Which kernel
// runs is decided before, once per step (fgx_select.h); this header only launches it.  What the units
// export is declared in fgx_launch.h.
#pragma once
#include <string>

#include "fgx_launch.h"
#include "fgx_ws.h"
#include "fgx_v2.h"
#include "fgx_select.h"

namespace fgx {

template <int MP, int NL, int NB>
static int launch_jp(const DevCfg& c, const DevState& s, const float* params, const Outputs& o, hipStream_t stream,
                     std::string& err) {
  const size_t lj = jp_lds_bytes<NL>(c.rows, c.stride);
  if (lj > 160 * 1024) {
    err = "k_episode_jp: basis table too large for LDS";
    return -4;
  }
  if (raise_lds_limit((const void*)k_episode_jp<MP, NL, NB>, lj) != hipSuccess) {
    err = "k_episode_jp: cannot raise the dynamic LDS limit";
    return -2;
  }
  hipLaunchKernelGGL((k_episode_jp<MP, NL, NB>), dim3((unsigned)((c.N + 63) / 64)), dim3(NL * 64), lj, stream, c, s,
                     params, o);
  return launch_status("k_episode_jp launch", err);
}

template <int MP, int NL, int NB>
static int launch_ws(const DevCfg& c, const DevState& s, const float* params, const Outputs& o, hipStream_t stream,
                     std::string& err) {
  const size_t lw = ws_lds_bytes<NL>(c.rows, c.stride);
  if (lw > 160 * 1024) {
    err = "k_episode_ws: basis table too large for LDS";
    return -4;
  }
  if (raise_lds_limit((const void*)k_episode_ws<MP, NL, NB>, lw) != hipSuccess) {
    err = "k_episode_ws: cannot raise the dynamic LDS limit";
    return -2;
  }
  const int64_t per_block = 64 * kWsPairs;
  hipLaunchKernelGGL((k_episode_ws<MP, NL, NB>), dim3((unsigned)((c.N + per_block - 1) / per_block)), dim3(512), lw,
                     stream, c, s, params, o);
  return launch_status("k_episode_ws launch", err);
}

// Launches the episode kernel `kernel` (EK_*, chosen once per step by select_episode_kernel,
// fgx_select.h); each case stands inside the condition under which this unit instantiates that
// kernel, and an id without an instantiation here is an error, never another kernel.
// LOG_ONLY (n_links outside {2, 5}, fgx_ep_nl.h): only the logging k_episode is instantiated; it
// serves every info level (no per-step array given: nothing is staged or stored) and the validity
// checks, so each further link count costs one kernel per (env, MP, controller), not a family.
template <int ENV, int MP, int CTRL, int NL, int NB, bool LOG_ONLY = false>
static int launch_episode_nl(const DevCfg& c, const DevState& s, int kernel, const float* params, const float* dpos,
                             const float* dvel, const Outputs& o, hipStream_t stream, std::string& err) {
  const int threads = 256;
  const int blocks = (int)((c.N + threads - 1) / threads);
  const size_t lds = (MP == MP_GIVEN) ? 0 : (size_t)c.rows * c.stride * sizeof(float);
  if constexpr (MP != MP_GIVEN && NB != 0) {
    if (c.stride != Traj<MP, 1, NB>::KS) {
      err = "basis table stride does not match the compiled layout";
      return -1;
    }
  }
  // SimpleReacher + PD on generated plans: k_episode_v2 and the shard kernels
  constexpr bool SIMPLE_PD = !LOG_ONLY && ENV == ENV_SIMPLE && MP != MP_GIVEN && CTRL == CTRL_PD;
  switch (kernel) {
    case EK_V2:
      if constexpr (SIMPLE_PD) {
        const size_t lv = v2_lds_bytes(c.rows, c.stride, NL);
        if (raise_lds_limit((const void*)k_episode_v2<MP, NL, NB>, lv) != hipSuccess) {
          err = "k_episode_v2: cannot raise the dynamic LDS limit";
          return -2;
        }
        hipLaunchKernelGGL((k_episode_v2<MP, NL, NB>), dim3((unsigned)((c.N + 64 * kV2Pairs - 1) / (64 * kV2Pairs))),
                           dim3(kV2Threads), lv, stream, c, s, params, o);
        return launch_status("k_episode_v2 launch", err);
      }
      break;
    case EK_JP:
      if constexpr (SIMPLE_PD) return launch_jp<MP, NL, NB>(c, s, params, o, stream, err);
      break;
    case EK_WS:
      if constexpr (SIMPLE_PD) return launch_ws<MP, NL, NB>(c, s, params, o, stream, err);
      break;
    case EK_JL:
      if constexpr (SIMPLE_PD) return fgx_launch_episode_jl(c, s, MP, NB, params, o, stream, err);
      break;
    case EK_PAIR:
      if constexpr (!LOG_ONLY && ENV == ENV_HOLE && NL == 5) {
        const int pblocks = (int)((2 * c.N + threads - 1) / threads);
        hipLaunchKernelGGL((k_episode_pair<ENV, MP, CTRL, NL, NB>), dim3(pblocks), dim3(threads), lds, stream, c, s,
                           params, dpos, dvel, o);
        return launch_status("k_episode_pair launch", err);
      }
      break;
    case EK_CLASSIC_W2:
      if constexpr (!LOG_ONLY && ENV == ENV_SIMPLE && NL == 5) {
        hipLaunchKernelGGL((k_episode_w2<ENV, MP, CTRL, NL, NB, false>), dim3(blocks), dim3(threads), lds, stream, c,
                           s, params, dpos, dvel, o);
        return launch_status("k_episode_w2 launch", err);
      }
      break;
    case EK_V2H:
      if constexpr (!LOG_ONLY && ENV != ENV_SIMPLE) {
        const size_t lh = v2h_lds_bytes(MP, c.rows, c.stride, NL, c.full_dim);
        if (raise_lds_limit((const void*)k_episode_v2h<ENV, MP, CTRL, NL, NB>, lh) != hipSuccess) {
          err = "k_episode_v2h: cannot raise the dynamic LDS limit";
          return -2;
        }
        hipLaunchKernelGGL((k_episode_v2h<ENV, MP, CTRL, NL, NB>), dim3((unsigned)(c.N / 256)), dim3(512), lh, stream,
                           c, s, params, dpos, dvel, o);
        return launch_status("k_episode_v2h launch", err);
      }
      break;
    case EK_CLASSIC:
      // the logging instantiation also runs the trajectory-validity checks (c.valid_flags)
      if (LOG_ONLY || episode_logs(c, o)) {
        if (ENV == ENV_SIMPLE && o.step_obs && !o.qlog) {
          err = "SimpleReacher per-step observations need the qlog scratch (fgx_step attaches it)";
          return -1;
        }
        // + the four waves' info staging regions (InfoStage, fgx_device.h)
        const size_t ll = stage_tab_offset(lds / sizeof(float)) + (threads / 64) * stage_wave_bytes(NL, c.full_dim);
        if (raise_lds_limit((const void*)k_episode<ENV, MP, CTRL, NL, NB, true>, ll) != hipSuccess) {
          err = "k_episode (info rows): cannot raise the dynamic LDS limit";
          return -2;
        }
        hipLaunchKernelGGL((k_episode<ENV, MP, CTRL, NL, NB, true>), dim3(blocks), dim3(threads), ll, stream, c, s,
                           params, dpos, dvel, o);
        if constexpr (ENV == ENV_SIMPLE) {
          if (o.qlog && o.step_obs) {   // the observation trigonometry of the logged rows (k_info_obs)
            if (const int rc = launch_status("k_episode launch", err)) return rc;
            hipLaunchKernelGGL((k_info_obs<NL>), dim3(blocks, c.T), dim3(threads), 0, stream, c, o);
          }
        }
        return launch_status("k_episode launch", err);
      }
      if constexpr (!LOG_ONLY) {
        hipLaunchKernelGGL((k_episode<ENV, MP, CTRL, NL, NB, false>), dim3(blocks), dim3(threads), lds, stream, c, s,
                           params, dpos, dvel, o);
        return launch_status("k_episode launch", err);
      }
      break;
  }
  err = "episode kernel not instantiated in this unit";
  return -4;
}

// NLV > 0: that link count only (the per-link-count units of fgx_ep_nl.h, logging kernel only);
// NLV = 0: the registered 2 and 5
template <int ENV, int MP, int CTRL, int NB, int NLV = 0>
static int launch_episode_ctrl(const DevCfg& c, const DevState& s, int kernel, const float* params,
                               const float* dpos, const float* dvel, const Outputs& o, hipStream_t stream,
                               std::string& err) {
  if constexpr (NLV > 0) {
    if (c.nl == NLV) return launch_episode_nl<ENV, MP, CTRL, NLV, NB, true>(c, s, kernel, params, dpos, dvel, o, stream, err);
  } else {
    if (c.nl == 2) return launch_episode_nl<ENV, MP, CTRL, 2, NB>(c, s, kernel, params, dpos, dvel, o, stream, err);
    if (c.nl == 5) return launch_episode_nl<ENV, MP, CTRL, 5, NB>(c, s, kernel, params, dpos, dvel, o, stream, err);
  }
  err = "n_links not instantiated in this unit";
  return -4;
}

template <int ENV, int MP, int NB, int NLV = 0>
static int launch_episode_mp(const DevCfg& c, const DevState& s, int kernel, const float* params, const float* dpos,
                             const float* dvel, const Outputs& o, hipStream_t stream, std::string& err) {
  switch (c.ctrl) {
    case CTRL_PD: return launch_episode_ctrl<ENV, MP, CTRL_PD, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
    case CTRL_VEL: return launch_episode_ctrl<ENV, MP, CTRL_VEL, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
    case CTRL_POS: return launch_episode_ctrl<ENV, MP, CTRL_POS, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
  }
  err = "bad ctrl_kind";
  return -1;
}

// NB = 5: every MP kind and the caller-given trajectory; NB = 0: the MP kinds with c.nb != 5 (and,
// in the per-link-count units NLV > 0, every basis count and the caller-given trajectory)
template <int ENV, int NB, int NLV = 0>
static int launch_episode_env(const DevCfg& c, const DevState& s, int mp, int kernel, const float* params,
                              const float* dpos, const float* dvel, const Outputs& o, hipStream_t stream,
                              std::string& err) {
  switch (mp) {
    case MP_PROMP: return launch_episode_mp<ENV, MP_PROMP, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
    case MP_DMP: return launch_episode_mp<ENV, MP_DMP, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
    case MP_PRODMP: return launch_episode_mp<ENV, MP_PRODMP, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
    case MP_GIVEN:
      // (if constexpr: the NB = 0 units of 2 / 5 links do not compile a second caller-given family)
      if constexpr (NB == 5 || NLV > 0)
        return launch_episode_mp<ENV, MP_GIVEN, NB, NLV>(c, s, kernel, params, dpos, dvel, o, stream, err);
      break;
  }
  err = "bad mp kind";
  return -1;
}

}  // namespace fgx
