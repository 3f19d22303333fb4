// fgx_seq_nl.h — k_rollout_seq for a handle of FGX_NL links (fgx_rollout_bb_seq, include/fgx.h).
// Included once by each fgx_seq_nl<n>.hip, which defines FGX_NL: a unit of its own per link count, so
// that the forms compile beside the count's other kernel families (fgx_ep_nl<n>.hip) instead of after
// them -- no unit lasts longer than the slowest episode unit (build time).
// fgx_ep_nl.h puts fgx_launch_rollout_seq_<n> into the count's NlOps table.
// The forms are nl_rollout_bb's: NB = 5 beside the generic basis count for the registered link counts 2
// and 5, the generic count alone for the others; k_rollout_bb's grid (C * ceil(N / 256) workgroups of
// 256 envs of one candidate) and LDS (the shared basis table).
#pragma once
#include "fgx_kernels.h"
#include "fgx_launch.h"
#include "fgx_nl_pick.h"

#define FGX_NL_CAT2(a, b) a##b
#define FGX_NL_CAT(a, b) FGX_NL_CAT2(a, b)

int FGX_NL_CAT(fgx_launch_rollout_seq_, FGX_NL)(const fgx::DevCfg& c, const fgx::DevState& s, const float* params,
                                                int n_seg, int n_cand, const fgx::Outputs& o, int32_t* segments,
                                                double* seg_ret, int32_t* seg_len, hipStream_t stream,
                                                std::string& err) {
  using namespace fgx;
  constexpr int NL = FGX_NL;
  const int64_t blocks = (int64_t)n_cand * ((c.N + 255) / 256);
  if (blocks > 0x7fffffff) {
    err = "k_rollout_seq: n_cand * ceil(n_envs / 256) workgroups exceed the grid limit";
    return -4;
  }
  const size_t lds = (size_t)c.rows * c.stride * sizeof(float);
  return pick<ENV_SIMPLE, ENV_HOLE, ENV_VIA>(c.env, -1, "bad env kind", err, [&](auto ENV) {
    return pick<CTRL_PD, CTRL_VEL, CTRL_POS>(c.ctrl, -1, "bad ctrl_kind", err, [&](auto CTRL) {
      return pick_mp_nb<NL>(c, "fgx_rollout_bb_seq needs a movement primitive", err, [&](auto MP, auto NB) {
        if constexpr (NB != 0) {
          if (c.stride != Traj<MP, 1, NB>::KS) {
            err = "basis table stride does not match the compiled layout";
            return -1;
          }
        }
        return launch("k_rollout_seq launch", k_rollout_seq<ENV, MP, CTRL, NL, NB>, dim3((unsigned)blocks), dim3(256),
                      lds, stream, err, c, s, params, o, n_seg, n_cand, segments, seg_ret, seg_len);
      });
    });
  });
}
