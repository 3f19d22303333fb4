// Host build of csrc/fgx_npsum.h (tests/test_wide_host.py): reads rows of f64 values from a file of
// records [int64 n][int64 rows][rows * n doubles] and writes np_sum_pairwise of each row, as raw doubles.
// A third argument "256" sums with np_sum_pairwise_256 instead (the episode kernels' return, n <= 256).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../fancy_gym_crowd_amd/csrc/fgx_npsum.h"

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) return 2;
  const bool le256 = argc == 4 && std::strcmp(argv[3], "256") == 0;
  if (argc == 4 && !le256) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int64_t hdr[2];
  std::vector<double> buf;
  while (std::fread(hdr, sizeof(int64_t), 2, in) == 2) {
    const int n = (int)hdr[0];
    const int64_t rows = hdr[1];
    buf.resize((size_t)n * rows);
    if (std::fread(buf.data(), sizeof(double), buf.size(), in) != buf.size()) return 4;
    for (int64_t r = 0; r < rows; ++r) {
      const double* a = buf.data() + (size_t)r * n;
      if (le256 && n > 256) return 5;
      auto get = [&](int i) { return a[i]; };
      const double s = le256 ? fgx::np_sum_pairwise_256(get, n) : fgx::np_sum_pairwise(get, n);
      std::fwrite(&s, sizeof(double), 1, out);
    }
  }
  std::fclose(in);
  std::fclose(out);
  return 0;
}
