// vgicp_resident_plan.h — what the calls over the resident scan at a pose ask of a context, and what
// vgicp_evaluate_resident and vgicp_align_resident_batch refuse, in their order.  Pure functions of plain facts (no HIP
// call, no context), so that a CPU program can enumerate them (tests/native/resident_plan.cpp).  The per-point report
// and the gated insertion decide likewise (vgicp_points_plan.h, vgicp_map_plan.h): their facts begin with ResidentFacts.
#pragma once
#include <cstdint>

#include "../../include/vgicp_hip_batch.h"
#include "../../include/vgicp_hip_evaluate.h"

namespace vgicp {

// What each of these calls asks of a context (resident_facts(ctx), vgicp_capi_resident.inl).  An entry plans twice: with
// the facts as it finds them, and again once what was pending has been settled: n is the resident scan's size only then.
struct ResidentFacts {
  bool several_devices = false;   // a multi-device context, one of its sub-contexts, a communicator or a peer-connected context
  bool has_map = true;
  bool scan_resident = true;
  bool settled = false;
  uint64_t n = 0;
};
struct ResidentVerdict {
  int rule = 0;                 // of the entry's list; 0: not refused
  int status = VGICP_OK;
  const char* text = nullptr;   // status != VGICP_OK (rule 1 has no context to leave it in)
  bool forward = false;         // plan_batch: not refused, and the multi-device context's to run
};
// The last three rules of both lists (first, first + 1, first + 2): a map, a scan, and after settling still a scan.
constexpr const char* kNoScanText = "no scan resident: call vgicp_scan_upload first";   // vgicp_align_batch_width's too
inline ResidentVerdict plan_ready(const ResidentFacts& f, int first) {
  if (!f.has_map) return {first, VGICP_ERR_NOT_READY, "no voxel map: call vgicp_map_reset first"};
  if (!f.scan_resident && !f.settled) return {first + 1, VGICP_ERR_NOT_READY, kNoScanText};
  if (!f.scan_resident) return {first + 2, VGICP_ERR_NOT_READY, "no scan resident"};
  return {};
}

// ---- vgicp_evaluate_resident (include/vgicp_hip_evaluate.h), rules 1 .. 8 ----
struct EvaluateFacts {
  bool ctx = true, poses = true, out = true;   // not NULL
  uint64_t k = 1;
  int64_t bad_pose = -1;                       // the first of the k poses with an entry that is not finite, or -1
  ResidentFacts at;
};
inline ResidentVerdict plan_evaluate(const EvaluateFacts& f) {
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT};
  if (f.k < 1 || f.k > VGICP_EVAL_MAX) return {2, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_EVAL_MAX"};
  if (!f.poses || !f.out) return {3, VGICP_ERR_BAD_ARGUMENT, "NULL pointer"};
  if (f.bad_pose >= 0) return {4, VGICP_ERR_BAD_ARGUMENT, " has an entry that is not finite"};   // behind "pose <bad_pose>"
  if (f.at.several_devices)
    return {5, VGICP_ERR_BAD_ARGUMENT, "vgicp_evaluate_resident is not available on multi-device contexts, communicators "
                                       "and peer-connected contexts: the resident scan of a device is a shard there"};
  return plan_ready(f.at, 6);
}

// ---- vgicp_align_resident_batch (include/vgicp_hip_batch.h), rules 1 .. 8; 4 and 5 are check_params' ----
struct BatchFacts {
  bool ctx = true, guesses = true, out_poses = true, params = true;   // not NULL
  uint64_t k = 1;
  int max_iteration = 0;
  bool multi = false;   // the handle IS a multi-device context: it runs the batch itself, as k aligns of the group
  ResidentFacts at;
};
inline ResidentVerdict plan_batch(const BatchFacts& f) {
  if (!f.ctx) return {1, VGICP_ERR_BAD_ARGUMENT};
  if (f.k < 1 || f.k > VGICP_BATCH_MAX) return {2, VGICP_ERR_BAD_ARGUMENT, "k must be 1 .. VGICP_BATCH_MAX"};
  if (!f.guesses || !f.out_poses) return {3, VGICP_ERR_BAD_ARGUMENT, "NULL pose pointer"};
  if (!f.params) return {4, VGICP_ERR_BAD_ARGUMENT, "params is NULL"};
  if (f.max_iteration < 0) return {5, VGICP_ERR_BAD_ARGUMENT, "max_iteration < 0"};
  ResidentVerdict v = f.multi ? ResidentVerdict{} : plan_ready(f.at, 6);
  v.forward = f.multi;   // a route, not a refusal: it comes before what a single context is asked
  return v;
}

}  // namespace vgicp
