// pick (csrc/fgx_launch.h: a run-time kind -> the std::integral_constant of the listed value that
// equals it) on the CPU, run by tests/test_host_pick.py: one line per case, compared with lines the
// test writes down from pick's contract.  No device is needed.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <string>

#include "../../fancy_gym_crowd_amd/csrc/fgx_launch.h"

using namespace fgx;

static int g_calls;   // calls of the innermost callable

// The shape of the episode ladder: MP kind, controller, link count, a bool.  The callable returns its
// four tags as one number, so a tag that is not its own value shows in the result.
static int ladder(int mp, int ctrl, int nl, int b, std::string& err) {
  return pick<MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN>(mp, -1, "bad mp kind", err, [&](auto MP) {
    return pick<CTRL_PD, CTRL_VEL, CTRL_POS>(ctrl, -1, "bad ctrl_kind", err, [&](auto CTRL) {
      return pick<2, 5>(nl, -4, "not instantiated", err, [&](auto NL) {
        return pick<0, 1>(b, -3, "not a bool", err, [&](auto B) {
          static_assert(MP >= MP_PROMP && MP <= MP_GIVEN && CTRL >= CTRL_PD && CTRL <= CTRL_POS && (NL == 2 || NL == 5) &&
                        (B == 0 || B == 1), "the tags are compile-time constants");
          ++g_calls;
          return MP * 1000 + CTRL * 100 + NL * 10 + B;
        });
      });
    });
  });
}

static void run_ladder(int mp, int ctrl, int nl, int b) {
  std::string err = "untouched";
  g_calls = 0;
  const int rc = ladder(mp, ctrl, nl, b, err);
  std::printf("ladder mp=%d ctrl=%d nl=%d b=%d -> rc=%d calls=%d err=%s\n", mp, ctrl, nl, b, rc, g_calls, err.c_str());
}

template <int... Vs>
static void run_flat(const char* list, int v) {
  std::string err = "untouched";
  int calls = 0, tag = -99;
  const int rc = pick<Vs...>(v, -7, "miss", err, [&](auto V) {
    ++calls;
    tag = V;
    return 40 + V;
  });
  std::printf("flat <%s> v=%d -> rc=%d tag=%d calls=%d err=%s\n", list, v, rc, tag, calls, err.c_str());
}

int main() {
  // every listed value reaches its own tag, four levels deep
  for (int mp : {MP_PROMP, MP_DMP, MP_PRODMP, MP_GIVEN})
    for (int ctrl : {CTRL_PD, CTRL_VEL, CTRL_POS})
      for (int nl : {2, 5})
        for (int b : {0, 1}) run_ladder(mp, ctrl, nl, b);
  // a value outside the list: at the outer level, and at each inner level under hits outside it
  for (int mp : {(int)MP_NONE, 5, -1}) run_ladder(mp, CTRL_PD, 5, 0);
  for (int ctrl : {3, -1}) run_ladder(MP_DMP, ctrl, 2, 1);
  for (int nl : {1, 3, 8}) run_ladder(MP_PRODMP, CTRL_VEL, nl, 0);
  run_ladder(MP_GIVEN, CTRL_POS, 5, 2);
  run_ladder(MP_NONE, 3, 3, 2);   // (the outermost miss reports)
  // one level: hits, misses, a repeated value, one value
  for (int v : {5, 0, 4}) run_flat<5, 0>("5, 0", v);
  for (int v : {0, 5}) run_flat<0, 0>("0, 0", v);
  for (int v : {3, 7, 2}) run_flat<3, 7, 3, 7>("3, 7, 3, 7", v);
  for (int v : {6, 0}) run_flat<6>("6", v);
  return 0;
}
