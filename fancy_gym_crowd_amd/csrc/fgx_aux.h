// fgx_aux.h — state (de)serialisation kernels.
#pragma once
#include <string>

#include "fgx_device.h"

namespace fgx {

// SoA [k][N] <-> row-major [N, k]
__global__ void k_get_state(DevCfg c, DevState s, double* q, double* qd, double* goal, double* hole, int32_t* steps) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= c.N) return;
  const int64_t N = c.N;
  for (int k = 0; k < c.nl; ++k) {
    if (q) q[e * c.nl + k] = s.q[k * N + e];
    if (qd) qd[e * c.nl + k] = s.qd[k * N + e];
  }
  if (goal) { goal[2 * e] = s.goal[e]; goal[2 * e + 1] = s.goal[N + e]; }
  if (hole) for (int k = 0; k < 3; ++k) hole[3 * e + k] = s.hole[k * N + e];
  if (steps) steps[e] = s.steps[e];
}

__global__ void k_set_state(DevCfg c, DevState s, const double* q, const double* qd, const double* goal,
                            const double* hole, const int32_t* steps) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= c.N) return;
  const int64_t N = c.N;
  for (int k = 0; k < c.nl; ++k) {
    if (q) s.q[k * N + e] = q[e * c.nl + k];
    if (qd) s.qd[k * N + e] = qd[e * c.nl + k];
  }
  if (goal) { s.goal[e] = goal[2 * e]; s.goal[N + e] = goal[2 * e + 1]; }
  if (hole) for (int k = 0; k < 3; ++k) s.hole[k * N + e] = hole[3 * e + k];
  if (steps) s.steps[e] = steps[e];
}

}  // namespace fgx

inline int fgx_transpose_state(const fgx::DevCfg& c, const fgx::DevState& s, double* q, double* qd, double* goal,
                               double* hole, int32_t* steps, hipStream_t stream, std::string& err) {
  const int threads = 256;
  const int blocks = (int)((c.N + threads - 1) / threads);
  return fgx::launch("k_get_state", fgx::k_get_state, dim3(blocks), dim3(threads), 0, stream, err, c, s, q, qd, goal, hole,
                     steps);
}

inline int fgx_untranspose_state(const fgx::DevCfg& c, const fgx::DevState& s, const double* q, const double* qd,
                                 const double* goal, const double* hole, const int32_t* steps, hipStream_t stream,
                                 std::string& err) {
  const int threads = 256;
  const int blocks = (int)((c.N + threads - 1) / threads);
  return fgx::launch("k_set_state", fgx::k_set_state, dim3(blocks), dim3(threads), 0, stream, err, c, s, q, qd, goal, hole,
                     steps);
}
