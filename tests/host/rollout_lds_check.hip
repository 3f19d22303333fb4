// Host build of csrc/fgx_rollout_lds.h (tests/test_rollout_host.py): prints, for every
// "dof obs_dim" pair on the command line, one line "dof obs_dim chunk stride wave_floats lds_bytes".
#include <cstdio>
#include <cstdlib>

#include "../../fancy_gym_crowd_amd/csrc/fgx_rollout_lds.h"

int main(int argc, char** argv) {
  if (argc < 3 || argc % 2 != 1) return 2;
  for (int i = 1; i + 1 < argc; i += 2) {
    const int dof = std::atoi(argv[i]), od = std::atoi(argv[i + 1]);
    std::printf("%d %d %d %d %d %d\n", dof, od, fgx::rollout_chunk(dof), fgx::rollout_stride(dof),
                fgx::rollout_wave_floats(dof, od), fgx::rollout_lds_bytes(dof, od));
  }
  return 0;
}
