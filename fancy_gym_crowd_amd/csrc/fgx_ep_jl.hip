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
  hipLaunchKernelGGL((fgx::k_episode_jl<MP, NL, NB>), dim3(blocks), dim3(S::THREADS + 64 * rw), S::lds_bytes(),
                     stream, c, s, params, o, gw, rw);
  return fgx::launch_status("k_episode_jl launch", err);
}

template <int MP, int NB>
int launch_jl_nl(const fgx::DevCfg& c, const fgx::DevState& s, const float* params, const fgx::Outputs& o,
                 hipStream_t stream, std::string& err) {
  // the helper form (a joint wave and a helper wave per workgroup, FGX_JL_HELPER=1 / 2) measured slower
  // at every shard size and was removed: asking for it is an error, not the plain form
  if (const char* v = std::getenv("FGX_JL_HELPER"))
    if (v[0] == '1' || v[0] == '2') {
      err = "k_episode_jl: FGX_JL_HELPER asks for the helper form, which was removed (DESIGN.md 4.6a)";
      return -4;
    }
  if (c.nl == 2) return launch_jl<MP, 2, NB>(c, s, params, o, stream, err);
  if (c.nl == 5) return launch_jl<MP, 5, NB>(c, s, params, o, stream, err);
  err = "k_episode_jl: n_links not instantiated (supported: 2, 5)";
  return -4;
}

template <int NB>
int launch_jl_mp(const fgx::DevCfg& c, const fgx::DevState& s, int mp, const float* params, const fgx::Outputs& o,
                 hipStream_t stream, std::string& err) {
  switch (mp) {
    case fgx::MP_PROMP: return launch_jl_nl<fgx::MP_PROMP, NB>(c, s, params, o, stream, err);
    case fgx::MP_DMP: return launch_jl_nl<fgx::MP_DMP, NB>(c, s, params, o, stream, err);
    case fgx::MP_PRODMP: return launch_jl_nl<fgx::MP_PRODMP, NB>(c, s, params, o, stream, err);
  }
  err = "k_episode_jl: bad mp kind";
  return -1;
}
}  // namespace

int fgx_launch_episode_jl(const fgx::DevCfg& c, const fgx::DevState& s, int mp, int nbs, const float* params,
                          const fgx::Outputs& o, hipStream_t stream, std::string& err) {
  if (nbs == 5) return launch_jl_mp<5>(c, s, mp, params, o, stream, err);
  if (nbs == 0) return launch_jl_mp<0>(c, s, mp, params, o, stream, err);
  err = "k_episode_jl: basis count not instantiated";
  return -4;
}
