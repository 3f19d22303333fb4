// fgx_nl_pick.h — the compiled basis counts of a link count and the pick of MP kind and basis count,
// shared by the units of one link count (fgx_ep_nl.h, fgx_seq_nl.h).
#pragma once
#include "fgx_launch.h"

namespace {
using namespace fgx;
template <int NL>
constexpr bool kRegistered = NL == 2 || NL == 5;
// the compiled basis count besides the generic NB = 0 (the registered counts: 5; the others: none)
template <int NL>
constexpr int kNB5 = kRegistered<NL> ? 5 : 0;

// f(MP, NB): the tags of the handle's MP kind and of the compiled basis count that serves c.nb
// (kNB5<NL>, else the generic 0); no MP: -1 with `miss`
template <int NL, class F>
int pick_mp_nb(const DevCfg& c, const char* miss, std::string& err, F&& f) {
  return pick<MP_PROMP, MP_DMP, MP_PRODMP>(c.mp, -1, miss, err, [&](auto MP) {
    return pick<kNB5<NL>, 0>(c.nb == kNB5<NL> ? c.nb : 0, -1, miss, err, [&](auto NB) { return f(MP, NB); });
  });
}
}  // namespace
