// fgx_wide.h — k_traj_wide: the desired trajectories of a wide handle as an f32 MFMA GEMM.
//
// Past the dozen basis functions the episode kernels keep in registers, the plan contraction
//   Y[k, (e, d)] = sum_j H[k + 1][j] * C[(e, d)][j]          (H: the shared table, s0 = 0)
// is a real GEMM: [T x K] table times [K x N dof] coefficients, K = n_basis (ProMP) or n_basis + 3
// (ProDMP: weights, goal, c1, c2), up to 1024.  It runs on v_mfma_f32_32x32x2_f32, whose numerics
// are bit for bit the k-ordered fmaf chain (cdna_hip_programming.md §3, fgx_mfma.h), so the plans
// equal oracle/mp.py:trajectory's: the K loop walks the columns in ascending k from a +0
// accumulator, and zero pads stand only behind the last real column (odd K: the last
// instruction's second slot is 0 * 0).  Operand maps as in fgx_mfma.h: lane l holds
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; D: col = l & 31,
// row = (r & 3) + 8 (r >> 2) + 4 (l >> 5) for accumulator register r.
//
// Layout.  The columns are flat: column (e, d) of B is the contiguous run
// params[(e dof + d) cs .. + Kw) with cs = Kw = n_basis (ProMP) or n_basis + 1 (ProDMP), so the link
// count is a run-time number and one kernel per MP kind serves every handle.  A workgroup of 8 waves
// owns a group of 16 envs (at most 128 columns = 4 column blocks of 32) and walks the groups; wave w
// owns the 32-row tile of plan samples 32 w .. 32 w + 31 (T <= 256) and keeps one accumulator per
// column block (ProDMP: a second set for the velocity basis).  Per 32-wide K slab:
//   * B: the group's slab is fetched from HBM into registers one slab ahead, coalesced along the
//     parameter axis (32 consecutive lanes read 128 consecutive bytes of one column), and written to
//     LDS [column][33]; every wave reads its B operands from there;
//   * A: each lane reads the slab of its table row from the L2-resident shared table (one cache line
//     per row and slab); the table is never staged whole into LDS;
//   * ProDMP: one thread per column runs the row-0 chains P, V over the staged slab on the VALU (the
//     same k-ordered chain); behind the last slab c1, c2 follow from the 2 x 2 system of
//     fgx_mfma.h and enter as the last B columns.
// Each table row is contracted once.  The positions are staged in LDS as whole env runs
// [env][T][dof] and leave with 16-B stores; ProMP's velocities are formed from the staged positions
// on the way out (vel_k = (pos_{k+1} - pos_k) / dt32 of row k + 1, the last sample repeats
// vel_{T-2}), ProDMP's are the second accumulator set divided by tau, staged after the positions left.
#pragma once
#include "fgx_launch.h"

namespace fgx {

typedef float wide_f32x16 __attribute__((ext_vector_type(16)));
typedef float wide_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWideWaves = 8;    // waves = 32-row tiles per workgroup (T <= 256)
constexpr int kWideGE = 16;      // envs per group
constexpr int kWideCB = 4;       // 32-column blocks per group: 16 envs x 8 links = 128 columns
constexpr int kWideCols = 32 * kWideCB;
constexpr int kWideKS = 32;      // K slab width
constexpr int kWideBS = kWideKS + 1;   // LDS floats per column of the B slab (odd: bank spread)
constexpr int kWideThreads = 64 * kWideWaves;
constexpr int kWideFetch = kWideCols * kWideKS / kWideThreads;   // slab floats per thread

// LDS floats of one env's staged run [T][dof] (16-B aligned rows of the region)
__host__ __device__ inline int wide_env_stride(int T, int dof) { return ((T * dof + 3) & ~3) + 4; }
inline size_t traj_wide_lds_bytes(int T, int dof) {
  return sizeof(float) * ((size_t)kWideGE * wide_env_stride(T, dof) + (size_t)kWideCols * kWideBS + kWideCols * 4);
}

// vec: the runs are 16-B aligned in dpos / dvel (T dof % 4 == 0, aligned bases): 16-B stores
template <int MP>
__global__ __launch_bounds__(kWideThreads) void k_traj_wide(DevCfg c, DevState s, const float* __restrict__ params,
                                                            float* __restrict__ dpos, float* __restrict__ dvel,
                                                            int vec) {
  constexpr bool PRO = MP == MP_PROMP;
  constexpr int GE = kWideGE, CB = kWideCB, KS = kWideKS, BS = kWideBS;
  extern __shared__ float4 lds_wide[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int64_t N = c.N;
  const int T = c.T, dof = c.nl, nb = c.nb, stride = c.stride;
  const int run = T * dof;                       // floats of one env's [T][dof] run
  const int ESR = wide_env_stride(T, dof);
  float* reg = (float*)lds_wide;                 // [GE][ESR] staged runs
  float* bs = reg + GE * ESR;                    // [128][BS] B slab
  float* tailb = bs + kWideCols * BS;            // [128][4] ProDMP: the B columns behind the slabs
  const float* tab = s.tables;
  const int Kw = PRO ? nb : nb + 1;              // B columns that come from params (= their stride there)
  const int Ktot = PRO ? nb : nb + 3;            // all columns
  // the pairs (k, k + 1), k even, k < Kmain run in the slab loop: ProMP all of them (odd nb: the last
  // slot is the 0 * 0 pad), ProDMP those that lie inside the params columns
  const int Kmain = PRO ? (nb + 1) & ~1 : Kw & ~1;
  const int tb = 32 * wave;                      // the wave's first plan sample
  const bool has_tile = tb < T;
  // this lane feeds plan sample tb + j of the tile: table row + 1 (rows past the plan repeat the last)
  const float* ar = tab + (size_t)(min(tb + j, T - 1) + 1) * stride;
  const int64_t groups = (N + GE - 1) / GE;

  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int64_t e0 = grp * GE;
    const int nenv = (int)min((int64_t)GE, N - e0);
    const int ncols = nenv * dof;                // (<= 128)
    const int ncb = (ncols + 31) >> 5;
    const float* pg = params + e0 * c.n_params;  // column cc: pg + cc * Kw

    wide_f32x16 ap[CB], av[PRO ? 1 : CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) {
      const wide_f32x16 z = {0.0f};
      ap[u] = z;
      if constexpr (!PRO) av[u] = z;
    }
    float P = 0.0f, V = 0.0f;                    // ProDMP: thread tid < ncols, row-0 chains of column tid

    // the slab [k0, k0 + KS) of the group's columns: element i * 512 + tid = (column, k - k0), k fastest
    float pre[kWideFetch];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < kWideFetch; ++i) {
        const int idx = i * kWideThreads + tid;
        const int kq = idx & (KS - 1), cc = idx >> 5, k = k0 + kq;
        pre[i] = (cc < ncols && k < Kw) ? pg[(size_t)cc * Kw + k] : 0.0f;
      }
    };
    fetch(0);
    for (int k0 = 0; k0 < Kw; k0 += KS) {
      // The lane's A values of the slab, loaded before anything else of the iteration: the table's L2
      // latency passes behind the staging, and the loads stand ahead of the next slab's fetch in the
      // wave's load queue (loads return in order: an A load issued behind the fetch would make the
      // contraction wait for HBM every slab).  Unconditional, so that they issue back to back.
      float a1v[KS / 2], a2v[PRO ? 1 : KS / 2];
      if (has_tile) {
#pragma unroll
        for (int q = 0; q < KS / 2; ++q) {
          const int kh = k0 + 2 * q + h;
          a1v[q] = kh < Kw ? ar[kh] : 0.0f;
          if constexpr (!PRO) a2v[q] = kh < Kw ? ar[nb + 1 + kh] : 0.0f;
        }
      }
      lds_barrier();   // the previous slab's readers are done (and the previous group's region readers)
#pragma unroll
      for (int i = 0; i < kWideFetch; ++i) {
        const int idx = i * kWideThreads + tid;
        const int kq = idx & (KS - 1), cc = idx >> 5, k = k0 + kq;
        float x = pre[i];
        if constexpr (!PRO) {
          x = x * (k < nb ? c.ws32 : c.gs32);    // (k > nb: 0)
          if (k == nb) tailb[cc * 4] = x;        // the goal column, should it open the tail (Kw odd)
        }
        bs[cc * BS + kq] = x;
      }
      lds_barrier();
      if (k0 + KS < Kw) fetch(k0 + KS);          // in flight during this slab's contraction
      if constexpr (!PRO) {
        if (tid < ncols) {
          const float* bc = bs + tid * BS;
          const int m = min(KS, Kw - k0);
          for (int kq = 0; kq < m; ++kq) {
            P = __builtin_fmaf(tab[k0 + kq], bc[kq], P);
            V = __builtin_fmaf(tab[nb + 1 + k0 + kq], bc[kq], V);
          }
        }
      }
      if (has_tile) {
#pragma unroll
        for (int q = 0; q < KS / 2; ++q) {
          const int kk = 2 * q;
          if (k0 + kk < Kmain) {                 // (wave-uniform)
#pragma unroll
            for (int u = 0; u < CB; ++u)
              if (u < ncb) {
                const float b = bs[(32 * u + j) * BS + kk + h];
                ap[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v[q], b, ap[u], 0, 0, 0);
                if constexpr (!PRO) av[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2v[q], b, av[u], 0, 0, 0);
              }
          }
        }
      }
    }

    if constexpr (!PRO) {
      // c1, c2 of every column from the boundary condition at step 0 (oracle/mp.py, fgx_mfma.h), then
      // the columns behind the slabs: Kw even: (c1, c2); Kw odd: (goal, c1), (c2, 0)
      if (tid < kWideCols) {
        float* tbc = tailb + tid * 4;
        if (tid < ncols) {
          const int je = tid / dof, d = tid - je * dof;
          const int64_t e = e0 + je;
          const float y1 = tab[2 * nb + 2], y2 = tab[2 * nb + 3], dy1 = tab[2 * nb + 4], dy2 = tab[2 * nb + 5];
          const float det = y1 * dy2 - y2 * dy1;
          const float A = (float)s.q[d * N + e] - P;
          const float B = (float)s.qd[d * N + e] * c.tau32 - V;
          const float c1 = (dy2 * A - y2 * B) / det;
          const float c2 = (y1 * B - dy1 * A) / det;
          const int o = Kw & 1;
          tbc[o] = c1;
          tbc[o + 1] = c2;
          if (!o) tbc[2] = 0.0f;
          tbc[3] = 0.0f;
        } else {
          tbc[0] = tbc[1] = tbc[2] = tbc[3] = 0.0f;
        }
      }
      lds_barrier();
      if (has_tile) {
        const int kr = Kw & ~1;
        for (int t = 0; kr + 2 * t < Ktot; ++t) {
          const int k = kr + 2 * t + h;
          // position basis [pb_0 .. pb_nb, y1, y2], velocity basis [vb_0 .. vb_nb, dy1, dy2]
          const float a1 = k <= nb ? ar[k] : (k < Ktot ? ar[2 * nb + 2 + (k - nb - 1)] : 0.0f);
          const float a2 = k <= nb ? ar[nb + 1 + k] : (k < Ktot ? ar[2 * nb + 4 + (k - nb - 1)] : 0.0f);
#pragma unroll
          for (int u = 0; u < CB; ++u)
            if (u < ncb) {
              const float b = tailb[(32 * u + j) * 4 + 2 * t + h];
              ap[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, ap[u], 0, 0, 0);
              av[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b, av[u], 0, 0, 0);
            }
        }
      }
    }

    // the wave's tile into the region [env][T][dof]: lane (j, h) holds column 32 u + j, rows
    // (r & 3) + 8 (r >> 2) + 4 h of the tile
    auto stage = [&](const wide_f32x16* v, bool by_tau) __attribute__((always_inline)) {
      if (!has_tile) return;
#pragma unroll
      for (int u = 0; u < CB; ++u) {
        const int col = 32 * u + j;
        if (u < ncb && col < ncols) {
          const int je = col / dof, d = col - je * dof;
          float* dst = reg + je * ESR + d;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int k = tb + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (k < T) dst[k * dof] = by_tau ? div_rcp(v[u][r], c.tau32, c.rcp_tau32) : v[u][r];
          }
        }
      }
    };
    // the staged runs to out, whole env runs: wave w streams envs w, w + 8
    auto store_runs = [&](float* out) __attribute__((always_inline)) {
      for (int je = wave; je < nenv; je += kWideWaves) {
        const float* src = reg + je * ESR;
        float* dst = out + (e0 + je) * run;
        if (vec) {
          for (int ch = lane; ch < (run >> 2); ch += 64)
            *reinterpret_cast<wide_f32x4*>(dst + 4 * ch) = *reinterpret_cast<const wide_f32x4*>(src + 4 * ch);
        } else {
          for (int i = lane; i < run; i += 64) dst[i] = src[i];
        }
      }
    };
    // ProMP: the velocities from the staged positions (fgx_mfma.h:138-144's rules)
    auto store_vel_promp = [&](float* out) __attribute__((always_inline)) {
      for (int je = wave; je < nenv; je += kWideWaves) {
        const float* src = reg + je * ESR;
        float* dst = out + (e0 + je) * run;
        auto vel_at = [&](int i) __attribute__((always_inline)) {
          const int k = i / dof;
          const bool last = k >= T - 1;
          const float* dr = tab + (size_t)(last ? T - 1 : k + 1) * stride + nb;   // dt32, 1 / dt32
          const float x = last ? src[i] - src[i - dof] : src[i + dof] - src[i];
          return div_rcp(x, dr[0], dr[1]);
        };
        if (vec) {
          for (int ch = lane; ch < (run >> 2); ch += 64) {
            const int i = 4 * ch;
            *reinterpret_cast<wide_f32x4*>(dst + i) = wide_f32x4{vel_at(i), vel_at(i + 1), vel_at(i + 2), vel_at(i + 3)};
          }
        } else {
          for (int i = lane; i < run; i += 64) dst[i] = vel_at(i);
        }
      }
    };

    stage(ap, false);
    lds_barrier();
    store_runs(dpos);
    if constexpr (PRO) {
      store_vel_promp(dvel);
    } else {
      lds_barrier();   // every wave's position reads done before the velocities overwrite the region
      stage(av, true);
      lds_barrier();
      store_runs(dvel);
    }
  }
}

// the plans [N, T dof] into info's time- and component-major arrays [T dof, N] (64 x 64 tiles)
__global__ __launch_bounds__(256) void k_plan_info(int64_t N, int run, const float* __restrict__ dpos,
                                                   const float* __restrict__ dvel, float* __restrict__ ipos,
                                                   float* __restrict__ ivel) {
  __shared__ float tp[64][65], tv[64][65];
  const int64_t e0 = (int64_t)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
  for (int r = y; r < 64; r += 4) {
    const int64_t e = e0 + r;
    const int kd = k0 + x;
    if (e < N && kd < run) {
      tp[r][x] = dpos[e * run + kd];
      tv[r][x] = dvel[e * run + kd];
    }
  }
  __syncthreads();
  for (int r = y; r < 64; r += 4) {
    const int64_t e = e0 + x;
    const int kd = k0 + r;
    if (e < N && kd < run) {
      ipos[(int64_t)kd * N + e] = tp[x][r];
      ivel[(int64_t)kd * N + e] = tv[x][r];
    }
  }
}

}  // namespace fgx
