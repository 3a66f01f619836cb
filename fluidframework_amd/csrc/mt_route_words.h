// mt_route_words.h — a route (mt_route.h) as words: the export format of the test hooks that let Python read
// the program (runtime.cpp fmt_internal_mt_route, tests/emu emu_mt_route; parsed by native.parse_mt_route).
#pragma once

#include <vector>

#include "mt_route.h"

namespace fmt_plan {

// A route as words, for the test hooks that let Python read it (fmt_internal_mt_route, emu_mt_route):
// tiersCkpt, largeCkpt, largeResumesSmall, largeHugeCkpt, largeLocal, the large variant's key, rounds,
// nominalLaunches for (largeRan, grew) = (0, 0), (1, 0), (0, 1), (1, 1), the number of steps; then per
// step kRouteStepWords words: tier, variant key, in / up / down as (kind, r, k) each, orderInto's kind,
// deal as (kind, r, k), descend; then the number of kMtKernels entries and each as (tier, variant key).
constexpr size_t kRouteHeadWords = 12, kRouteStepWords = 16;
inline std::vector<uint32_t> routeWords(const MtRoute& R) {
  std::vector<uint32_t> w{R.tiersCkpt, R.largeCkpt, R.largeResumesSmall, R.largeHugeCkpt, R.largeLocal, R.large.key(),
                          static_cast<uint32_t>(R.rounds), R.nominalLaunches(false, false), R.nominalLaunches(true, false),
                          R.nominalLaunches(false, true), R.nominalLaunches(true, true), static_cast<uint32_t>(R.nSteps)};
  for (int i = 0; i < R.nSteps; i++) {
    const MtStep& s = R.steps[i];
    w.insert(w.end(), {static_cast<uint32_t>(s.tier), s.variant.key()});
    for (const MtList& l : {s.in, s.up, s.down}) w.insert(w.end(), {static_cast<uint32_t>(l.kind), l.r, l.k});
    w.insert(w.end(), {static_cast<uint32_t>(s.orderInto.kind), static_cast<uint32_t>(s.deal.kind), s.deal.r, s.deal.k, s.descend});
  }
  w.push_back(static_cast<uint32_t>(sizeof kMtKernels / sizeof kMtKernels[0]));
  for (const MtKernelId& k : kMtKernels) w.insert(w.end(), {static_cast<uint32_t>(k.tier), k.variant.key()});
  return w;
}

}  // namespace fmt_plan
