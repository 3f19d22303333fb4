// The snapshot blob layout (csrc/fgx_snapshot.h: snapshot_layout) on the CPU, run by
// tests/test_snapshot_host.py: a table of DevCfg / DevState values (env kind, link count, the
// optional aux and cond arrays present or absent, env count), one line per case with the blob size
// and every section's offset, bytes per env and presence.  The program checks the layout's
// invariants itself (exit status 1 and a message on the first violation); the test checks the
// printed numbers again against the formula written in Python.  snapshot_layout is a pure host
// function, so no device is needed; the state pointers are never dereferenced.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

// ---- the function under test
#include "../../fancy_gym_crowd_amd/csrc/fgx_snapshot.h"

using namespace fgx;

static const char* const kEnv[] = {"simple", "hole", "via"};
static const char* const kSec[kSnapSections] = {"q", "qd", "goal", "hole", "aux", "steps", "plans", "flags", "rng", "cond",
                                                "start"};

#define REQUIRE(cond, ...)                  \
  do {                                      \
    if (!(cond)) {                          \
      std::fprintf(stderr, __VA_ARGS__);    \
      std::fprintf(stderr, " (%s)\n", #cond); \
      std::exit(1);                         \
    }                                       \
  } while (0)

static void emit(int env, int nl, bool aux, bool cond, long N) {
  DevCfg c = {};
  c.N = N;
  c.env = env;
  c.nl = nl;
  // any non-null address marks an array as allocated
  static double arr;
  DevState s = {};
  s.q = s.qd = s.goal = s.hole = s.start = &arr;
  s.aux = aux ? &arr : nullptr;
  s.steps = s.plans = (int32_t*)&arr;
  s.flags = (uint32_t*)&arr;
  s.rng = (uint64_t*)&arr;
  s.cond = cond ? (float*)&arr : nullptr;
  const SnapLayout L = snapshot_layout(c, s);

  const int bpe[kSnapSections] = {8 * nl, 8 * nl, 16, 24, 24, 4, 4, 4, 40, 8 * nl, 8};
  size_t end = 0, total = 0;
  for (int k = 0; k < kSnapSections; ++k) {
    const SnapSection& x = L.sec[k];
    const bool want = (k == SEC_AUX) ? aux : (k == SEC_COND ? cond : true);
    REQUIRE(x.present == want, "%s: presence", kSec[k]);
    REQUIRE(x.bytes_per_env() == (want ? bpe[k] : 0), "%s: bytes per env %d", kSec[k], x.bytes_per_env());
    REQUIRE(x.offset % 256 == 0, "%s: offset %zu not 256-byte aligned", kSec[k], x.offset);
    REQUIRE(x.offset >= end, "%s: offset %zu overlaps the section before it (ends at %zu)", kSec[k], x.offset, end);
    if (!want) continue;   // (no space: the next section may start at the same offset)
    end = x.offset + (size_t)x.bytes_per_env() * (size_t)N;
    total += ((size_t)bpe[k] * (size_t)N + 255) / 256 * 256;
    REQUIRE(end <= L.bytes, "%s: ends at %zu past the blob (%zu)", kSec[k], end, L.bytes);
  }
  REQUIRE(L.bytes == total, "blob of %zu bytes, formula %zu", L.bytes, total);

  std::printf("%s nl=%d aux=%d cond=%d N=%ld bytes=%zu", kEnv[env], nl, (int)aux, (int)cond, N, L.bytes);
  for (int k = 0; k < kSnapSections; ++k)
    std::printf(" %s=%zu:%d:%d", kSec[k], L.sec[k].offset, L.sec[k].bytes_per_env(), (int)L.sec[k].present);
  std::printf("\n");
}

int main() {
  for (int env : {ENV_SIMPLE, ENV_HOLE, ENV_VIA})
    for (int nl : {1, 2, 5, 8})
      for (bool aux : {false, true})
        for (bool cond : {false, true})
          for (long N : {1L, 67L, 256L}) emit(env, nl, aux, cond, N);
  return 0;
}
