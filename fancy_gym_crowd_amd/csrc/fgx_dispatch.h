// fgx_dispatch.h — the episode kernels of one env kind and basis specialisation: launch_episode_env
// picks the MP kind, controller and link count (pick, fgx_launch.h), launch_episode_nl launches the
// kernel chosen once per step (fgx_select.h) through launch (fgx_device.h).  One translation unit per
// env kind and basis specialisation for 2 / 5 links (fgx_ep_<env>.hip: NB = 5, the registered configs;
// fgx_ep_<env>_gen.hip: NB = 0, the generic runtime basis count) and one per further link count
// (fgx_ep_nl.h, the logging kernel only), so that the build compiles them in parallel.  The `if
// constexpr` conditions here state what a unit instantiates.  What the units export is declared in
// fgx_launch.h.
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
  return launch("k_episode_jp launch", k_episode_jp<MP, NL, NB>, dim3((unsigned)((c.N + 63) / 64)), dim3(NL * 64), lj,
                stream, err, c, s, params, o);
}

template <int MP, int NL, int NB>
static int launch_ws(const DevCfg& c, const DevState& s, const float* params, const Outputs& o, hipStream_t stream,
                     std::string& err) {
  const size_t lw = ws_lds_bytes<NL>(c.rows, c.stride);
  if (lw > 160 * 1024) {
    err = "k_episode_ws: basis table too large for LDS";
    return -4;
  }
  const int64_t per_block = 64 * kWsPairs;
  return launch("k_episode_ws launch", k_episode_ws<MP, NL, NB>, dim3((unsigned)((c.N + per_block - 1) / per_block)),
                dim3(512), lw, stream, err, c, s, params, o);
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
        return launch("k_episode_v2 launch", k_episode_v2<MP, NL, NB>,
                      dim3((unsigned)((c.N + 64 * kV2Pairs - 1) / (64 * kV2Pairs))), dim3(kV2Threads), lv, stream, err, c,
                      s, params, o);
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
        return launch("k_episode_pair launch", k_episode_pair<ENV, MP, CTRL, NL, NB>, dim3(pblocks), dim3(threads), lds,
                      stream, err, c, s, params, dpos, dvel, o);
      }
      break;
    case EK_CLASSIC_W2:
      if constexpr (!LOG_ONLY && ENV == ENV_SIMPLE && NL == 5)
        return launch("k_episode_w2 launch", k_episode_w2<ENV, MP, CTRL, NL, NB, false>, dim3(blocks), dim3(threads), lds,
                      stream, err, c, s, params, dpos, dvel, o);
      break;
    case EK_V2H:
      if constexpr (!LOG_ONLY && ENV != ENV_SIMPLE) {
        const size_t lh = v2h_lds_bytes(MP, c.rows, c.stride, NL, c.full_dim);
        return launch("k_episode_v2h launch", k_episode_v2h<ENV, MP, CTRL, NL, NB>, dim3((unsigned)(c.N / 256)),
                      dim3(512), lh, stream, err, c, s, params, dpos, dvel, o);
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
        const int rc = launch("k_episode launch", k_episode<ENV, MP, CTRL, NL, NB, true>, dim3(blocks), dim3(threads), ll,
                              stream, err, c, s, params, dpos, dvel, o);
        if constexpr (ENV == ENV_SIMPLE) {
          if (rc == 0 && o.qlog && o.step_obs)   // the observation trigonometry of the logged rows (k_info_obs)
            return launch("k_episode launch", k_info_obs<NL>, dim3(blocks, c.T), dim3(threads), 0, stream, err, c, o);
        }
        return rc;
      }
      if constexpr (!LOG_ONLY)
        return launch("k_episode launch", k_episode<ENV, MP, CTRL, NL, NB, false>, dim3(blocks), dim3(threads), lds,
                      stream, err, c, s, params, dpos, dvel, o);
      break;
  }
  err = "episode kernel not instantiated in this unit";
  return -4;
}

// NB = 5: every MP kind and the caller-given trajectory; NB = 0: the MP kinds with c.nb != 5 (and,
// in the per-link-count units NLV > 0, every basis count and the caller-given trajectory).
// NLV > 0: that link count only (the per-link-count units of fgx_ep_nl.h, logging kernel only);
// NLV = 0: the registered 2 and 5
template <int ENV, int NB, int NLV = 0>
static int launch_episode_env(const DevCfg& c, const DevState& s, int mp, int kernel, const float* params,
                              const float* dpos, const float* dvel, const Outputs& o, hipStream_t stream,
                              std::string& err) {
  return pick<MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN>(mp, -1, "bad mp kind", err, [&](auto MP) {
    // (the NB = 0 units of 2 / 5 links do not compile a second caller-given family)
    if constexpr (MP == MP_GIVEN && NB != 5 && NLV == 0) {
      err = "bad mp kind";
      return -1;
    } else {
      return pick<CTRL_PD, CTRL_VEL, CTRL_POS>(c.ctrl, -1, "bad ctrl_kind", err, [&](auto CTRL) {
        return pick<(NLV ? NLV : 2), (NLV ? NLV : 5)>(c.nl, -4, "n_links not instantiated in this unit", err, [&](auto NL) {
          return launch_episode_nl<ENV, MP, CTRL, NL, NB, (NLV > 0)>(c, s, kernel, params, dpos, dvel, o, stream, err);
        });
      });
    }
  });
}

}  // namespace fgx
