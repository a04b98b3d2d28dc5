// What vgicp_evaluate_resident and vgicp_align_resident_batch decide without the device
// (eskf_lio_amd/csrc/vgicp_resident_plan.h), on the CPU: plan_evaluate and plan_batch over every combination of their
// facts against the ordered lists restated here (the first line that applies names the rule, the status and the WHOLE
// text, as the entries had them inline), and the layout of the argument structs that begin with the pose view
// (vgicp_device.h, host side only): PoseView is the first 148 bytes of PointArgs and GateArgs, field for field.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "vgicp_device.h"
#include "vgicp_resident_plan.h"

using namespace vgicp;

namespace {
struct Want {
  int rule, status;
  std::string text;
};
const char* const kNoMap = "no voxel map: call vgicp_map_reset first";
const char* const kNoScan = "no scan resident: call vgicp_scan_upload first";

// include/vgicp_hip_evaluate.h's entry as it was written out: the first line that applies
Want evaluate_by_the_list(const EvaluateFacts& f) {
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT, ""};
  if (f.k == 0 || f.k > 64) return {2, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_EVAL_MAX"};
  if (!(f.poses && f.out)) return {3, VGICP_ERR_BAD_ARGUMENT, "NULL pointer"};
  if (f.bad_pose >= 0) return {4, VGICP_ERR_BAD_ARGUMENT, "pose " + std::to_string(f.bad_pose) + " has an entry that is not finite"};
  if (f.at.several_devices)
    return {5, VGICP_ERR_BAD_ARGUMENT,
            "vgicp_evaluate_resident is not available on multi-device contexts, communicators and peer-connected contexts: "
            "the resident scan of a device is a shard there"};
  if (!f.at.has_map) return {6, VGICP_ERR_NOT_READY, kNoMap};
  if (!f.at.settled && !f.at.scan_resident) return {7, VGICP_ERR_NOT_READY, kNoScan};
  if (f.at.settled && !f.at.scan_resident) return {8, VGICP_ERR_NOT_READY, "no scan resident"};
  return {0, VGICP_OK, ""};
}
// include/vgicp_hip_batch.h's likewise; forward: the multi-device context takes the batch before a map is asked for
Want batch_by_the_list(const BatchFacts& f, bool* forward) {
  *forward = false;
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT, ""};
  if (f.k == 0 || f.k > 64) return {2, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_BATCH_MAX"};
  if (!(f.guesses && f.out_poses)) return {3, VGICP_ERR_BAD_ARGUMENT, "NULL pose pointer"};
  if (!f.params) return {4, VGICP_ERR_BAD_ARGUMENT, "params is NULL"};
  if (f.max_iteration < 0) return {5, VGICP_ERR_BAD_ARGUMENT, "max_iteration < 0"};
  if (f.multi) {
    *forward = true;
    return {0, VGICP_OK, ""};
  }
  if (!f.at.has_map) return {6, VGICP_ERR_NOT_READY, kNoMap};
  if (!f.at.settled && !f.at.scan_resident) return {7, VGICP_ERR_NOT_READY, kNoScan};
  if (f.at.settled && !f.at.scan_resident) return {8, VGICP_ERR_NOT_READY, "no scan resident"};
  return {0, VGICP_OK, ""};
}
// rule, status, text (none iff not refused or rule 1) and the route.  before: what the host puts in front of the text
bool agrees(const ResidentVerdict& v, const Want& w, bool forward, const std::string& before = std::string()) {
  const bool has_text = v.text != nullptr;
  if (v.rule != w.rule || v.status != w.status || v.forward != forward || has_text != !w.text.empty()) return false;
  return !has_text || before + v.text == w.text;
}
ResidentFacts at_of(unsigned bits) {
  return ResidentFacts{(bits & 1u) != 0, (bits & 2u) != 0, (bits & 4u) != 0, (bits & 8u) != 0, (bits & 4u) ? 6000u : 0u};
}
}  // namespace

int main() {
  const uint64_t ks[] = {0, 1, 64, 65};
  unsigned long long checked = 0, seen[9] = {0};
  // ---- plan_evaluate ----
  const int64_t bad_poses[] = {-1, 0, 3, 63};
  for (unsigned bits = 0; bits < (1u << 7); ++bits)
    for (uint64_t k : ks)
      for (int64_t bad : bad_poses) {
        EvaluateFacts f;
        f.ctx = bits & 1u, f.poses = bits & 2u, f.out = bits & 4u;
        f.k = k, f.bad_pose = bad, f.at = at_of(bits >> 3);
        const ResidentVerdict v = plan_evaluate(f);
        if (!agrees(v, evaluate_by_the_list(f), false, v.rule == 4 ? "pose " + std::to_string(bad) : std::string())) {
          std::printf("plan_evaluate: facts %u k %llu bad pose %lld: rule %d status %d\n", bits, (unsigned long long)k, (long long)bad, v.rule, v.status);
          return 1;
        }
        ++seen[v.rule], ++checked;
      }
  for (int r = 0; r <= 8; ++r)
    if (!seen[r]) { std::printf("plan_evaluate: rule %d never turned up\n", r); return 1; }
  std::printf("evaluate ok %llu\n", checked);
  // ---- plan_batch ----
  const int max_iterations[] = {-1, 0, 10};
  unsigned long long forwarded = 0;
  checked = 0;
  for (unsigned long long& s : seen) s = 0;
  for (unsigned bits = 0; bits < (1u << 9); ++bits)
    for (uint64_t k : ks)
      for (int max_it : max_iterations) {
        BatchFacts f;
        f.ctx = bits & 1u, f.guesses = bits & 2u, f.out_poses = bits & 4u, f.params = bits & 8u, f.multi = bits & 16u;
        f.k = k, f.max_iteration = max_it, f.at = at_of(bits >> 5);
        bool forward = false;
        const Want w = batch_by_the_list(f, &forward);
        const ResidentVerdict v = plan_batch(f);
        if (!agrees(v, w, forward)) {
          std::printf("plan_batch: facts %u k %llu max_iteration %d: rule %d status %d forward %d\n", bits, (unsigned long long)k, max_it, v.rule, v.status, (int)v.forward);
          return 1;
        }
        ++seen[v.rule], ++checked, forwarded += v.forward;
      }
  for (int r = 0; r <= 8; ++r)
    if (!seen[r]) { std::printf("plan_batch: rule %d never turned up\n", r); return 1; }
  if (!forwarded) { std::printf("plan_batch: never forwarded\n"); return 1; }
  std::printf("batch ok %llu\n", checked);

  // ---- the pose view and the two argument structs that begin with it ----
#pragma GCC diagnostic ignored "-Winvalid-offsetof"
  static_assert(sizeof(ResidentView) == 40 && sizeof(PoseView) == 152, "the views");
  static_assert(offsetof(PoseView, pose) == 40 && offsetof(PoseView, asym_dev) == 136 && offsetof(PoseView, scan_seq) == 144, "PoseView");
  static_assert(sizeof(PointArgs) == 224 && offsetof(PointArgs, pose) == 40 && offsetof(PointArgs, asym_dev) == 136 &&
                offsetof(PointArgs, scan_seq) == 144 && offsetof(PointArgs, robust_kernel) == 148 &&
                offsetof(PointArgs, robust_scale2) == 152 && offsetof(PointArgs, counters) == 216, "PointArgs");
  static_assert(sizeof(GateArgs) == 176 && offsetof(GateArgs, pose) == 40 && offsetof(GateArgs, asym_dev) == 136 &&
                offsetof(GateArgs, scan_seq) == 144 && offsetof(GateArgs, pad) == 148 && offsetof(GateArgs, gate) == 152 &&
                offsetof(GateArgs, counters) == 168, "GateArgs");
  // assigning the view inside a struct leaves the field in the view's tail alone
  PointArgs a{};
  a.robust_kernel = 0x12345678u;
  PoseView v{};
  v.scan_seq = 7;
  static_cast<PoseView&>(a) = v;
  if (a.robust_kernel != 0x12345678u || a.scan_seq != 7) { std::printf("the view's tail\n"); return 1; }
  std::printf("layout ok %zu %zu %zu\n", sizeof(PoseView), sizeof(PointArgs), sizeof(GateArgs));
  return 0;
}
