// ViaPointReacher (direct velocity) instantiations of k_episode, NB = 5 (the registered basis count).
#include "fgx_dispatch.h"

int fgx_launch_episode_via(const fgx::DevCfg& c, const fgx::DevState& s, int mp, int kernel, const float* params,
                              const float* dpos, const float* dvel, const fgx::Outputs& o, hipStream_t stream,
                              std::string& err) {
  return fgx::launch_episode_env<fgx::ENV_VIA, 5>(c, s, mp, kernel, params, dpos, dvel, o, stream, err);
}
