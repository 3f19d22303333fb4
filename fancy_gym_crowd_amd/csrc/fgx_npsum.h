// fgx_npsum.h — np.sum of n f64 values in numpy's pairwise_sum order (umath loops_utils.h), for any n.
//
// The basis tables normalise each row by the sum of its n = n_basis + zero_start + zero_goal
// exponentials (oracle/mp.py:rbf64), and the tables equal the oracle's bit for bit only if that sum
// adds in numpy's order, which depends on n:
//   n < 8          left to right;
//   8 <= n <= 128  eight accumulators over the blocks of 8, combined as ((r0 + r1) + (r2 + r3)) +
//                  ((r4 + r5) + (r6 + r7)), then the n % 8 tail left to right;
//   n > 128        split at n2 = n / 2, n2 -= n2 % 8, and sum(first n2) + sum(rest), recursively.
// Stated once here, for the device (fgx_tables.h; fgx_device.h pairwise_strided, the episode return)
// and the host (tests/host/npsum_check.hip compiles this header alone and compares it with np.sum for
// every n in 1..1024, np_sum_pairwise_256 for every n in 1..256).  get(i) returns the i-th
// value; it is called once per element, in numpy's order within each leaf.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FGX_HD __host__ __device__
#else
#define FGX_HD
#endif

namespace fgx {

// one leaf: m <= 128 values from lo on
template <class G>
FGX_HD inline double np_sum_block(G&& get, int lo, int m) {
  if (m < 8) {
    double s = get(lo) + 0.0;
    for (int i = 1; i < m; ++i) s = s + get(lo + i);
    return s;
  }
  double r[8];   // (unrolled: the accumulators stay in registers in device code)
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = get(lo + j);
  int i = 8;
  for (; i < m - (m % 8); i += 8)
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = r[j] + get(lo + i + j);
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < m; ++i) s = s + get(lo + i);
  return s;
}

// n <= 256 without a frame stack (the episode kernels' return sum: a stack array would live in
// their scratch memory).  Two levels of the recursion serve these lengths: the first half n2 =
// (n / 2) & ~7 is at most 128, one leaf; the second half n - n2 is at most 136, and above 128 (n in
// 249..255) numpy splits it once more, into leaves of 64 and 65..71.
template <class G>
FGX_HD inline double np_sum_pairwise_256(G&& get, int n) {
  if (n <= 128) return np_sum_block(get, 0, n);
  int n2 = n / 2;
  n2 -= n2 % 8;
  const int m = n - n2;
  const double first = np_sum_block(get, 0, n2);
  if (m <= 128) return first + np_sum_block(get, n2, m);
  int m2 = m / 2;
  m2 -= m2 % 8;
  return first + (np_sum_block(get, n2, m2) + np_sum_block(get, n2 + m2, m - m2));
}

// any n >= 1: the recursion as a walk over an explicit stack (device code takes no recursion; 32
// frames serve every int n, the halves shrink to 128 within 24 levels)
template <class G>
FGX_HD inline double np_sum_pairwise(G&& get, int n) {
  if (n <= 128) return np_sum_block(get, 0, n);
  struct Frame { int lo, n, stage; double left; };
  Frame st[32];
  int sp = 0;
  st[0] = Frame{0, n, 0, 0.0};
  double ret = 0.0;
  while (sp >= 0) {
    Frame f = st[sp];
    if (f.n <= 128) {
      ret = np_sum_block(get, f.lo, f.n);
      --sp;
      continue;
    }
    int n2 = f.n / 2;
    n2 -= n2 % 8;
    if (f.stage == 0) {          // descend into the first half
      st[sp].stage = 1;
      st[++sp] = Frame{f.lo, n2, 0, 0.0};
    } else if (f.stage == 1) {   // first half done: keep it, descend into the second
      st[sp].left = ret;
      st[sp].stage = 2;
      st[++sp] = Frame{f.lo + n2, f.n - n2, 0, 0.0};
    } else {                     // both done
      ret = f.left + ret;
      --sp;
    }
  }
  return ret;
}

}  // namespace fgx
