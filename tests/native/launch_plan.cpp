// Which instantiation of a round kernel a launch takes (eskf_lio_amd/csrc/vgicp_launch_plan.h: plan_iterate, plan_close,
// plan_persistent and the three lists), enumerated on the CPU against the launchers' predicates as they were written out
// by hand before they became one function each — copied here as they stood in launch_iterate (with launch_iterate_prior),
// launch_close and launch_persistent, with `args.` read from plain variables and the template arguments of the kernel
// they launched returned as flags.
// EVERY combination of the boolean facts, every listed value of the numeric ones; nothing skipped.  Also: no list names an
// instantiation twice, every entry of every list is reached, and an accepted fact has exactly one entry.
#include <cstdint>
#include <cstdio>

#include "vgicp_launch_plan.h"

using namespace vgicp;

namespace old {
constexpr uint32_t kPersistWorkers = 512 - 64;
constexpr uint32_t kMemoBytesPerPoint = 512 * 16;   // kPersistWide * sizeof(int4)
constexpr uint32_t kPersistDynLds = 150 * 1024;
constexpr uint32_t kPrefetchBytes = kPersistWorkers * (16 + 6 * 16);   // sizeof(int4) + 6 * sizeof(double2)

struct Iterate { bool refused; int block; bool robust, prior; };
Iterate launch_iterate_prior(bool ROBUST, int block) {
  switch (block) {
    case 256: return {false, 256, ROBUST, true};
    case 512: return {false, 512, ROBUST, true};
    case 1024: return {false, 1024, ROBUST, true};
    default: return {true, 0, false, false};
  }
}
Iterate launch_iterate(uint32_t robust_kernel, double robust_gate, uint32_t prior_on, int block) {
  if (prior_on != 0) {
    return (robust_kernel != 0 || robust_gate > 0.0) ? launch_iterate_prior(true, block) : launch_iterate_prior(false, block);
  }
  if (robust_kernel != 0 || robust_gate > 0.0) {
    switch (block) {
      case 256: return {false, 256, true, false};
      case 512: return {false, 512, true, false};
      case 1024: return {false, 1024, true, false};
      default: return {true, 0, false, false};
    }
  }
  switch (block) {
    case 256: return {false, 256, false, false};
    case 512: return {false, 512, false, false};
    case 1024: return {false, 1024, false, false};
    default: return {true, 0, false, false};
  }
}

struct Close { bool refused; int block; bool prior; };
Close launch_close(uint32_t prior_on, int block) {
  if (prior_on != 0) {
    switch (block) {
      case 256: return {false, 256, true};
      case 512: return {false, 512, true};
      case 1024: return {false, 1024, true};
      default: return {true, 0, false};
    }
  }
  switch (block) {
    case 256: return {false, 256, false};
    case 512: return {false, 512, false};
    case 1024: return {false, 1024, false};
    default: return {true, 0, false};
  }
}

struct Persistent { bool refused; bool multi, stamps, many, robust, prior; size_t dyn; };
Persistent as(bool MULTI, bool STAMPS, bool MANY, bool ROBUST, bool PRIOR, size_t dyn) {
  return {false, MULTI, STAMPS, MANY, ROBUST, PRIOR, dyn};
}
Persistent launch_persistent(uint32_t world, bool has_stamps, uint32_t n, uint32_t grid, uint32_t memo_points, uint32_t stash_bytes,
                             double prefetch_margin, uint32_t robust_kernel, double robust_gate, uint32_t prior_on) {
  const Persistent invalid = {true, false, false, false, false, false, 0};
  size_t dyn = (size_t)memo_points * kMemoBytesPerPoint + (size_t)stash_bytes;
  if (prefetch_margin > 0.0) {
    if (dyn != 0) return invalid;
    dyn = kPrefetchBytes;
  }
  if (dyn > kPersistDynLds) return invalid;
  const bool multi = world > 1, stamps = has_stamps;
  const bool many = (uint64_t)n > (uint64_t)grid * kPersistWorkers;
  if (prior_on != 0) {
    if (multi) return invalid;
    if (robust_kernel != 0 || robust_gate > 0.0)
      return many ? as(false, false, true, true, true, dyn) : as(false, false, false, true, true, dyn);
    return many ? as(false, false, true, false, true, dyn) : as(false, false, false, false, true, dyn);
  }
  if (robust_kernel != 0 || robust_gate > 0.0) {
    if (multi) return invalid;
    return many ? as(false, false, true, true, false, dyn) : as(false, false, false, true, false, dyn);
  }
  if (many) {
    if (multi) return stamps ? as(true, true, true, false, false, dyn) : as(true, false, true, false, false, dyn);
    return stamps ? as(false, true, true, false, false, dyn) : as(false, false, true, false, false, dyn);
  }
  if (multi) return stamps ? as(true, true, false, false, false, dyn) : as(true, false, false, false, false, dyn);
  return stamps ? as(false, true, false, false, false, dyn) : as(false, false, false, false, false, dyn);
}
}  // namespace old

static unsigned long long visited = 0, refused = 0;
static unsigned long long iterate_hits[kIterateVariantCount], close_hits[kCloseVariantCount], persistent_hits[kPersistentVariantCount];

static int bad(const char* what) { std::printf("MISMATCH: %s\n", what); return 1; }

int main() {
  // no list names an instantiation twice
  for (int i = 0; i < kIterateVariantCount; ++i)
    for (int j = i + 1; j < kIterateVariantCount; ++j)
      if (kIterateVariants[i].block == kIterateVariants[j].block && kIterateVariants[i].robust == kIterateVariants[j].robust &&
          kIterateVariants[i].prior == kIterateVariants[j].prior) return bad("kIterateVariants has a duplicate");
  for (int i = 0; i < kCloseVariantCount; ++i)
    for (int j = i + 1; j < kCloseVariantCount; ++j)
      if (kCloseVariants[i].block == kCloseVariants[j].block && kCloseVariants[i].prior == kCloseVariants[j].prior)
        return bad("kCloseVariants has a duplicate");
  for (int i = 0; i < kPersistentVariantCount; ++i)
    for (int j = i + 1; j < kPersistentVariantCount; ++j) {
      const PersistentVariant &a = kPersistentVariants[i], &b = kPersistentVariants[j];
      if (a.multi == b.multi && a.stamps == b.stamps && a.many == b.many && a.robust == b.robust && a.prior == b.prior)
        return bad("kPersistentVariants has a duplicate");
    }

  const int blocks[] = {128, 256, 512, 1024};
  const uint32_t kernels[] = {0, 1}, priors[] = {0, 1}, worlds[] = {1, 2}, grids[] = {1, 2, 256};
  const uint32_t memos[] = {0, 3, 19}, stashes[] = {0, 100000, 200000};
  const double gates[] = {0.0, 9.0}, margins[] = {0.0, 0.015};

  // ---- one round of the loop and its closing launch ----
  for (int block : blocks)
    for (uint32_t kernel : kernels)
      for (double gate : gates)
        for (uint32_t prior : priors) {
          if (robust_selected(kernel, gate) != (kernel != 0 || gate > 0.0)) return bad("robust_selected");
          ++visited;
          const old::Iterate want = old::launch_iterate(kernel, gate, prior, block);
          const int v = plan_iterate(block, kernel, gate, prior != 0);
          if ((v == kLaunchRefused) != want.refused) return bad("plan_iterate: refusal");
          if (want.refused) ++refused;
          else {
            if (v < 0 || v >= kIterateVariantCount) return bad("plan_iterate: index");
            const IterateVariant& got = kIterateVariants[v];
            if (got.block != want.block || got.robust != want.robust || got.prior != want.prior) return bad("plan_iterate: flags");
            int matches = 0;
            for (const IterateVariant& e : kIterateVariants) matches += e.block == want.block && e.robust == want.robust && e.prior == want.prior;
            if (matches != 1) return bad("plan_iterate: not exactly one entry");
            ++iterate_hits[v];
          }
          ++visited;
          const old::Close wc = old::launch_close(prior, block);
          const int c = plan_close(block, prior != 0);
          if ((c == kLaunchRefused) != wc.refused) return bad("plan_close: refusal");
          if (wc.refused) ++refused;
          else {
            if (c < 0 || c >= kCloseVariantCount) return bad("plan_close: index");
            if (kCloseVariants[c].block != wc.block || kCloseVariants[c].prior != wc.prior) return bad("plan_close: flags");
            int matches = 0;
            for (const CloseVariant& e : kCloseVariants) matches += e.block == wc.block && e.prior == wc.prior;
            if (matches != 1) return bad("plan_close: not exactly one entry");
            ++close_hits[c];
          }
        }

  // ---- the persistent launch ----
  for (uint32_t world : worlds)
    for (int stamps = 0; stamps < 2; ++stamps)
      for (uint32_t grid : grids) {
        const uint32_t ns[] = {0, 1, 448 * grid, 448 * grid + 1};
        for (uint32_t n : ns)
          for (uint32_t memo : memos)
            for (uint32_t stash : stashes)
              for (double margin : margins)
                for (uint32_t kernel : kernels)
                  for (double gate : gates)
                    for (uint32_t prior : priors) {
                      ++visited;
                      const old::Persistent want = old::launch_persistent(world, stamps != 0, n, grid, memo, stash, margin, kernel, gate, prior);
                      PersistentFacts f;
                      f.world = world;
                      f.stamps = stamps != 0;
                      f.n = n;
                      f.grid = grid;
                      f.memo_points = memo;
                      f.stash_bytes = stash;
                      f.prefetch_margin = margin;
                      f.robust_kernel = kernel;
                      f.robust_gate = gate;
                      f.prior = prior != 0;
                      const PersistentPlan p = plan_persistent(f);
                      if ((p.variant == kLaunchRefused) != want.refused) return bad("plan_persistent: refusal");
                      if (want.refused) { ++refused; continue; }
                      if (p.variant < 0 || p.variant >= kPersistentVariantCount) return bad("plan_persistent: index");
                      const PersistentVariant& got = kPersistentVariants[p.variant];
                      if (got.multi != want.multi || got.stamps != want.stamps || got.many != want.many || got.robust != want.robust ||
                          got.prior != want.prior) return bad("plan_persistent: flags");
                      if ((size_t)p.dyn_lds != want.dyn) return bad("plan_persistent: dynamic LDS");
                      int matches = 0;
                      for (const PersistentVariant& e : kPersistentVariants)
                        matches += e.multi == want.multi && e.stamps == want.stamps && e.many == want.many && e.robust == want.robust &&
                                   e.prior == want.prior;
                      if (matches != 1) return bad("plan_persistent: not exactly one entry");
                      ++persistent_hits[p.variant];
                    }
      }

  const unsigned long long expected = 2ull * 4 * 2 * 2 * 2 + 2ull * 2 * 3 * 4 * 3 * 3 * 2 * 2 * 2 * 2;
  if (visited != expected) { std::printf("visited %llu combinations, expected %llu\n", visited, expected); return 1; }
  for (int i = 0; i < kIterateVariantCount; ++i) if (iterate_hits[i] == 0) { std::printf("iterate variant %d is never planned\n", i); return 1; }
  for (int i = 0; i < kCloseVariantCount; ++i) if (close_hits[i] == 0) { std::printf("close variant %d is never planned\n", i); return 1; }
  for (int i = 0; i < kPersistentVariantCount; ++i)
    if (persistent_hits[i] == 0) { std::printf("persistent variant %d is never planned\n", i); return 1; }
  std::printf("ok %llu combinations refused %llu iterate %d close %d persistent %d\n", visited, refused, kIterateVariantCount,
              kCloseVariantCount, kPersistentVariantCount);
  return 0;
}
