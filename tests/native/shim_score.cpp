// CPU check of the drop-in's choice by score (include/eskf_lio_shim/Registration.hpp): ICP::Evaluation's derived
// figures and ICP::selectBestByScore on hand-made values.  Compiled against the stand-in types; links nothing of the
// module (only static members and plain structs are used, the C ABI is never called).
#define ESKF_LIO_SHIM_FORCE_POD 1
#include <cmath>
#include <cstdio>
#include <vector>

#include "eskf_lio_shim/Registration.hpp"

using ESKF_LIO::ICP;

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static ICP::Hypothesis hyp(bool converged) {
  ICP::Hypothesis h;
  h.converged = converged;
  h.iterations = 3;
  return h;
}
static ICP::Evaluation eval(uint64_t points, uint64_t matched, double cost, double sq = 0.0) {
  ICP::Evaluation e;
  e.points = points;
  e.correspondences = matched;
  e.cost = cost;
  e.squaredError = sq;
  return e;
}

int main() {
  // the derived figures
  const ICP::Evaluation e = eval(1000, 800, 100.0, 8.0);
  CHECK(e.fitness() == 0.8);
  CHECK(e.inlierRmse() == 0.1);
  CHECK(e.score() == 100.0 + 11.345 * 200.0);
  CHECK(e.score(2.0) == 500.0);
  CHECK(e.score(0.0) == 100.0);
  const ICP::Evaluation none = eval(1000, 0, 0.0);
  CHECK(none.fitness() == 0.0 && none.inlierRmse() == 0.0 && none.score(1.0) == 1000.0);
  const ICP::Evaluation empty = eval(0, 0, 0.0);
  CHECK(empty.fitness() == 0.0 && empty.inlierRmse() == 0.0 && empty.score() == 0.0);
  // information(): the packed lower triangle mirrored into a symmetric 6 x 6
  ICP::Evaluation tri;
  for (size_t k = 0; k < 27; ++k) tri.normalEquations[k] = 1.0 + static_cast<double>(k);
  const std::array<double, 36> m = tri.information();
  int k = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c <= r; ++c, ++k) CHECK(m[r + 6 * c] == 1.0 + k && m[c + 6 * r] == 1.0 + k);

  // converged before unconverged, whatever the scores say
  {
    const std::vector<ICP::Hypothesis> h = {hyp(false), hyp(true), hyp(false)};
    const std::vector<ICP::Evaluation> s = {eval(1000, 1000, 1.0), eval(1000, 10, 900.0), eval(1000, 1000, 0.5)};
    CHECK(ICP::selectBestByScore(h, s) == 1);
  }
  // a fuller match beats a lower cost per match: 0.05 per match on 400 points against 0.12 per match on all 1000
  {
    const std::vector<ICP::Hypothesis> h = {hyp(true), hyp(true)};
    const std::vector<ICP::Evaluation> s = {eval(1000, 400, 0.05 * 400), eval(1000, 1000, 0.12 * 1000)};
    CHECK(s[0].cost / 400.0 < s[1].cost / 1000.0 && s[0].cost < s[1].cost);
    CHECK(ICP::selectBestByScore(h, s) == 1);
    CHECK(ICP::selectBestByScore(h, s, 0.0) == 0);   // without a charge for the misses the sparse match would win
  }
  // among equals the lowest score; ties to the lower index
  {
    const std::vector<ICP::Hypothesis> h = {hyp(true), hyp(true), hyp(true), hyp(true)};
    const std::vector<ICP::Evaluation> s = {eval(100, 100, 7.0), eval(100, 100, 5.0), eval(100, 100, 5.0), eval(100, 100, 6.0)};
    CHECK(ICP::selectBestByScore(h, s) == 1);
    const std::vector<ICP::Hypothesis> u = {hyp(false), hyp(false)};
    const std::vector<ICP::Evaluation> t = {eval(100, 90, 5.0), eval(100, 90, 5.0)};
    CHECK(ICP::selectBestByScore(u, t) == 0);
  }
  // one evaluation per hypothesis
  {
    bool threw = false;
    try {
      ICP::selectBestByScore({hyp(true), hyp(true)}, {eval(1, 1, 0.0)});
    } catch (const std::runtime_error &) {
      threw = true;
    }
    CHECK(threw);
  }
  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
