// k_episode_hp instantiations (fgx_hp.h): HoleReacher, 5 links, 5 basis functions, every MP kind and
// controller, one group per workgroup (small batches: spread over the CUs) or four (one per SIMD).
#include <cstdlib>

#include "fgx_hp.h"
#include "fgx_launch.h"

namespace fgx {

// k_episode_hp's INFO instantiation is needed: some per-step array of HoleReacher's info is written.
// Narrower than episode_logs (fgx_select.h): reward_dist / reward_ctrl are SimpleReacher's lists,
// which this kernel never writes, and the validity checks are never on here (k_episode_hp is only
// selected with valid_flags == 0)
static bool hp_info_rows(const Outputs& o) {
  return o.positions || o.step_actions || o.step_obs || o.step_rewards || o.is_collided || o.end_effector;
}

template <int MP, int CTRL, int G, bool INFO>
static int launch_hp(const DevCfg& c, const DevState& s, const float* params, const Outputs& o, hipStream_t stream,
                     std::string& err) {
  if (c.stride != Traj<MP, 1, 5>::KS) {
    err = "k_episode_hp: basis table stride does not match the compiled layout";
    return -1;
  }
  const size_t lds = hp_lds_bytes(5, G);
  const int64_t per = 64 * G;
  if (const int rc = launch("k_episode_hp launch", k_episode_hp<MP, CTRL, 5, 5, G, INFO>,
                            dim3((unsigned)((c.N + per - 1) / per)), dim3(192 * G), lds, stream, err, c, s, params, o))
    return rc;
  return launch("k_hp_finish launch", k_hp_finish<5, CTRL != CTRL_PD>, dim3((unsigned)((c.N + 255) / 256)), dim3(256), 0,
                stream, err, c, s, o);
}

}  // namespace fgx

// four groups per workgroup (one per SIMD, one workgroup per CU) once the batch fills every CU that
// way; one group per workgroup below (FGX_HP_G=1 / 4 forces)
int fgx_launch_episode_hp(const fgx::DevCfg& c, const fgx::DevState& s, int mp, const float* params,
                          const fgx::Outputs& o, hipStream_t stream, std::string& err) {
  using namespace fgx;
  if (c.nl != 5 || c.nb != 5) {
    err = "k_episode_hp: 5 links and 5 basis functions only";
    return -4;
  }
  int G = (c.N >= (int64_t)device_cus() * 256) ? 4 : 1;   // (a full round: 256 envs per CU)
  if (const char* v = std::getenv("FGX_HP_G")) G = std::atoi(v) == 4 ? 4 : 1;
  return pick<4, 1>(G, -4, "k_episode_hp: group count not instantiated", err, [&](auto GV) {
    return pick<MP_PROMP, MP_DMP, MP_PRODMP>(mp, -1, "k_episode_hp: bad mp kind", err, [&](auto MP) {
      return pick<CTRL_PD, CTRL_VEL, CTRL_POS>(c.ctrl, -1, "bad ctrl_kind", err, [&](auto CTRL) {
        return pick<0, 1>(hp_info_rows(o), -1, "", err, [&](auto INFO) {
#ifdef FGX_HP_ONLY_CFG3   // diagnostics builds (tools/unit_variant.py): config 3's instantiation only
          if constexpr (MP != MP_PRODMP || CTRL != CTRL_PD || INFO != 0 || GV != 4) {
            err = "FGX_HP_ONLY_CFG3 build";
            return -1;
          } else
#endif
          return launch_hp<MP, CTRL, GV, INFO != 0>(c, s, params, o, stream, err);
        });
      });
    });
  });
}
