// k_episode_jl instantiations (fgx_jl.h): SimpleReacher + PD, every MP kind, 2 / 5 links, the
// registered basis count (NB = 5) and the generic one (NB = 0).  A translation unit of its own so
// that the build compiles it in parallel with the k_episode units.
#include "fgx_dispatch.h"
#include "fgx_jl.h"

#include <algorithm>
#include <cstdlib>

namespace {
template <int MP, int NL, int NB>
int launch_jl(const fgx::DevCfg& c, const fgx::DevState& s, const float* params, const fgx::Outputs& o,
              hipStream_t stream, std::string& err) {
  using S = fgx::JlShape<NL>;
  if constexpr (NB != 0) {
    if (c.stride != fgx::Traj<MP, 1, NB>::KS) {
      err = "basis table stride does not match the compiled layout";
      return -1;
    }
  }
  int gw = S::G;   // (fewer envs per wave measured slower at every N: profiles/r02_jl_scan.jsonl)
  if (const char* v = std::getenv("FGX_JL_GW")) gw = std::max(1, std::min(S::G, std::atoi(v)));   // experiments
  const int64_t per_block = (int64_t)S::WAVES * gw;
  const unsigned blocks = (unsigned)((c.N + per_block - 1) / per_block);
  // the reset wave (fgx_jl.h) while every workgroup has a CU of its own (the 8-GPU shard: 8192 envs
  // 23.8-24.0 -> 21.9-22.2 us, config 2 22.4 -> 20.1 us); past that its fifth wave costs a workgroup
  // slot per CU (32768 envs 45.2 -> 48.2 us, profiles/r06_jl_resetwave_ab.log).  FGX_JL_RW=0 / 1: A/B
  int rw = blocks <= (unsigned)fgx::device_cus() ? 1 : 0;
  if (const char* v = std::getenv("FGX_JL_RW")) rw = v[0] == '1' ? 1 : 0;
  return fgx::launch("k_episode_jl launch", fgx::k_episode_jl<MP, NL, NB>, dim3(blocks), dim3(S::THREADS + 64 * rw),
                     S::lds_bytes(), stream, err, c, s, params, o, gw, rw);
}
}  // namespace

int fgx_launch_episode_jl(const fgx::DevCfg& c, const fgx::DevState& s, int mp, int nbs, const float* params,
                          const fgx::Outputs& o, hipStream_t stream, std::string& err) {
  using namespace fgx;
  return pick<5, 0>(nbs, -4, "k_episode_jl: basis count not instantiated", err, [&](auto NB) {
    return pick<MP_PROMP, MP_DMP, MP_PRODMP>(mp, -1, "k_episode_jl: bad mp kind", err, [&](auto MP) {
      // the helper form (a joint wave and a helper wave per workgroup, FGX_JL_HELPER=1 / 2) measured slower
      // at every shard size and was removed: asking for it is an error, not the plain form
      if (const char* v = std::getenv("FGX_JL_HELPER"))
        if (v[0] == '1' || v[0] == '2') {
          err = "k_episode_jl: FGX_JL_HELPER asks for the helper form, which was removed (DESIGN.md 4.6a)";
          return -4;
        }
      return pick<2, 5>(c.nl, -4, "k_episode_jl: n_links not instantiated (supported: 2, 5)", err, [&](auto NL) {
        return launch_jl<MP, NL, NB>(c, s, params, o, stream, err);
      });
    });
  });
}
