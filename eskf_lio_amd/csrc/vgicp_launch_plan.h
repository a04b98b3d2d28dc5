// vgicp_launch_plan.h — which instantiation of a round kernel a launch takes, decided in one place: the lists of the
// instantiations that exist, and plan_iterate / plan_close / plan_persistent, which pick one of them (or refuse) from
// plain facts.  No HIP call and no context, so that a CPU program can enumerate them (tests/native/launch_plan.cpp).
// vgicp_kernels.hip builds its tables of kernel pointers from these same lists: an instantiation exists, has its LDS
// limit raised and can be launched exactly when it is listed here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vgicp {

// THE definition of "this launch runs the robust round" (RobustArgs: a kernel other than none, or a gate on d^2).
constexpr bool robust_selected(uint32_t kernel, double gate) { return kernel != 0 || gate > 0.0; }

// ---- the persistent launch's LDS (512-thread workgroups, one per CU) ----
constexpr uint32_t kPersistWorkers = 512 - 64;
constexpr uint32_t kPersistWide = 512;  // point-carrying threads when a thread owns several points (wave 0 included)
constexpr uint32_t kMemoBytesPerPoint = kPersistWide * 16;  // an int4 per thread: 8 192
// dynamic LDS of the persistent launch: the CU's 160 KB minus the kernel's static use and a margin
constexpr uint32_t kPersistDynLds = 150 * 1024;
constexpr uint32_t kPrefetchBytes = kPersistWorkers * (16 + 6 * 16);  // an int4 + six double2 per worker: 50 176
// Dynamic LDS of a launch that remembers memo_points keys per thread and parks points in stash_bytes behind them.
constexpr uint64_t persistent_dyn_lds_bytes(uint32_t memo_points, uint32_t stash_bytes) {
  return (uint64_t)memo_points * kMemoBytesPerPoint + stash_bytes;
}
constexpr uint32_t persistent_max_dyn_lds_bytes() { return kPersistDynLds; }  // the most a launch plan ever asks for

// ---- the instantiations.  ROBUST: the weighted round; PRIOR: the pose prior in the solve; MULTI: the rank totals
// travel through the mailboxes; STAMPS: workgroup 0 records its phase times; MANY: a thread owns several points ----
struct IterateVariant { int block; bool robust, prior; };
struct CloseVariant { int block; bool prior; };   // the closing launch accumulates nothing: no robust form
struct PersistentVariant { bool multi, stamps, many, robust, prior; };

constexpr IterateVariant kIterateVariants[] = {
    {256, false, false}, {512, false, false}, {1024, false, false},
    {256, true, false},  {512, true, false},  {1024, true, false},
    {256, false, true},  {512, false, true},  {1024, false, true},
    {256, true, true},   {512, true, true},   {1024, true, true},
};
constexpr CloseVariant kCloseVariants[] = {
    {256, false}, {512, false}, {1024, false}, {256, true}, {512, true}, {1024, true},
};
// the robust round and the pose prior: one device, no stamps
constexpr PersistentVariant kPersistentVariants[] = {
    {false, false, false, false, false}, {false, false, true, false, false},
    {false, true, false, false, false},  {false, true, true, false, false},
    {true, false, false, false, false},  {true, false, true, false, false},
    {true, true, false, false, false},   {true, true, true, false, false},
    {false, false, false, true, false},  {false, false, true, true, false},
    {false, false, false, false, true},  {false, false, true, false, true},
    {false, false, false, true, true},   {false, false, true, true, true},
};
constexpr int kIterateVariantCount = (int)(sizeof(kIterateVariants) / sizeof(kIterateVariants[0]));
constexpr int kCloseVariantCount = (int)(sizeof(kCloseVariants) / sizeof(kCloseVariants[0]));
constexpr int kPersistentVariantCount = (int)(sizeof(kPersistentVariants) / sizeof(kPersistentVariants[0]));
static_assert(kIterateVariantCount == 12 && kCloseVariantCount == 6 && kPersistentVariantCount == 14, "the lists as they stand");

constexpr int kLaunchRefused = -1;   // the launcher answers hipErrorInvalidValue

// Index of the listed variant with these flags, or kLaunchRefused when there is none.
constexpr int find_iterate(int block, bool robust, bool prior) {
  for (int i = 0; i < kIterateVariantCount; ++i) {
    const IterateVariant& v = kIterateVariants[i];
    if (v.block == block && v.robust == robust && v.prior == prior) return i;
  }
  return kLaunchRefused;
}
constexpr int find_close(int block, bool prior) {
  for (int i = 0; i < kCloseVariantCount; ++i)
    if (kCloseVariants[i].block == block && kCloseVariants[i].prior == prior) return i;
  return kLaunchRefused;
}
constexpr int find_persistent(bool multi, bool stamps, bool many, bool robust, bool prior) {
  for (int i = 0; i < kPersistentVariantCount; ++i) {
    const PersistentVariant& v = kPersistentVariants[i];
    if (v.multi == multi && v.stamps == stamps && v.many == many && v.robust == robust && v.prior == prior) return i;
  }
  return kLaunchRefused;
}

// ---- one round of the loop, and the launch that closes it: refused for a block size that has no instantiation ----
constexpr int plan_iterate(int block, uint32_t robust_kernel, double robust_gate, bool prior) {
  return find_iterate(block, robust_selected(robust_kernel, robust_gate), prior);
}
constexpr int plan_close(int block, bool prior) { return find_close(block, prior); }

// ---- the persistent launch ----
struct PersistentFacts {
  uint32_t world = 1;            // ranks that exchange through the mailboxes
  bool stamps = false;           // the context records phase times (VGICP_DEBUG_STAMPS)
  uint32_t n = 0;                // points of the scan (or their upper bound)
  uint32_t grid = 1;             // workgroups
  uint32_t memo_points = 0;
  uint32_t stash_bytes = 0;
  double prefetch_margin = 0.0;
  uint32_t robust_kernel = 0;
  double robust_gate = 0.0;
  bool prior = false;
};
struct PersistentPlan {
  int variant = kLaunchRefused;  // index into kPersistentVariants
  uint32_t dyn_lds = 0;          // bytes of dynamic LDS
};
constexpr PersistentPlan plan_persistent(const PersistentFacts& f) {
  uint64_t dyn = persistent_dyn_lds_bytes(f.memo_points, f.stash_bytes);
  if (f.prefetch_margin > 0.0) {
    if (dyn != 0) return PersistentPlan{};   // the prefetch area shares the LDS of memo / stash
    dyn = kPrefetchBytes;
  }
  if (dyn > persistent_max_dyn_lds_bytes()) return PersistentPlan{};
  const bool multi = f.world > 1, robust = robust_selected(f.robust_kernel, f.robust_gate);
  if (multi && (robust || f.prior)) return PersistentPlan{};   // the weighted round and the pose prior: one device ...
  const bool stamps = f.stamps && !robust && !f.prior;         // ... and no stamps: the context's are ignored
  const bool many = (uint64_t)f.n > (uint64_t)f.grid * kPersistWorkers;
  return PersistentPlan{find_persistent(multi, stamps, many, robust, f.prior), (uint32_t)dyn};
}

}  // namespace vgicp
