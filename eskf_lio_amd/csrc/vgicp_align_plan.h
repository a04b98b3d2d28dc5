// vgicp_align_plan.h — which host path an align takes: ONE pure function of plain facts (no HIP call, no context), so
// that a CPU program can enumerate it (tests/native/align_plan.cpp).  DESIGN.md §4 has the table written from it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace vgicp {

constexpr uint32_t kPointsPerPass = 448;  // points one workgroup takes per pass: waves 1-7 of its 512 threads (vgicp_device.h)
constexpr uint32_t kPlanTeamsMax = 16;    // hypotheses per team launch: vgicp_device.h's kTeamsMax (asserted in vgicp_context.h)
constexpr int kBatchSlotRows = 64;   // rows of kSlots doubles per hypothesis of a batch: the final state, then up to 63 rounds of log

// One point per thread: the scan fits ONE pass of the persistent grid (else a thread owns several points, `MANY`).
inline bool one_point_per_thread(uint64_t n, uint32_t grid) { return n <= (uint64_t)grid * kPointsPerPass; }

enum class AlignCall {
  Upload,    // vgicp_align: the scan comes from host buffers
  Resident,  // vgicp_align_resident (and vgicp_align once its upload is enqueued)
  Batch,     // vgicp_align_resident_batch
  Group      // a multi-device context: one align over all its sub-contexts
};
enum class AlignPath {
  Fused,       // one launch that reads the staged upload itself
  Persistent,  // one persistent launch (Group: on every device, the rows through the mailboxes)
  Teams,       // one launch per `width` hypotheses
  Loop,        // one launch per round
  GroupLoop    // one launch per round on every device, the rows added on the host (a sub-context: left to its group)
};

struct AlignFacts {
  AlignCall call = AlignCall::Resident;
  // the call
  uint64_t n = 0;                // Upload: the caller's count; else the resident scan's (Batch: settled)
  size_t k = 1;                  // Batch: hypotheses
  int max_iteration = 0;
  bool profile = false, no_persistent = false;   // VGICP_FLAG_PROFILE, VGICP_FLAG_NO_PERSISTENT
  bool buffers = false;          // Upload: scan, guess and output pointers are all there
  bool upload_staged = false;    // Upload: the copy threads stage this scan (upload_is_staged)
  // the context (Group: persistent_enabled = on EVERY device, cooldown = the group's)
  bool persistent_enabled = false, owner = false, comm = false, peers_connected = false, peer_enabled = false;
  bool stamps = false, stage_events = false, no_fused = false;
  bool mailboxes = false;        // Group: the device-initiated exchange is wired
  int world_size = 1, peer_world = 1, cooldown = 0;
  uint32_t grid = 0;             // workgroups of every persistent launch
  bool robust = false;           // a robust kernel or a gate is set (include/vgicp_hip_robust.h)
  bool prior = false;            // a pose prior is set (include/vgicp_hip_prior.h): planned exactly as `robust` is
};

struct AlignPlan {
  AlignPath path = AlignPath::Loop;   // Upload, not Fused: the Resident call's; Batch, width 1: the first single align's
  bool peer_path = false;        // the launch exchanges rows with peer GPUs
  int cooldown_drop = 0;         // aligns this call takes off the cool-down
  uint32_t width = 1;            // Batch: hypotheses per launch; 1 = k single aligns, each planned as a Resident call
  uint32_t team_wgs = 0;         // Batch, width >= 2: workgroups per team
};

// Hypotheses one team launch takes for the resident scan (vgicp_align_batch_width): T = ceil(n / 448) workgroups per
// team, as many teams as fit the grid vgicp_create verified to be resident; 1 = no team launch.
inline uint32_t team_width(const AlignFacts& f, uint32_t* team_wgs) {
  *team_wgs = 0;
  if (f.robust || f.prior) return 1;   // the robust round and the pose prior have no team kernel
  const bool one_device = f.world_size == 1 && !f.owner && !f.comm && !f.peers_connected;
  if (!one_device || !f.persistent_enabled || f.stamps || f.n == 0 || !one_point_per_thread(f.n, f.grid)) return 1;
  const uint32_t T = (uint32_t)((f.n + kPointsPerPass - 1) / kPointsPerPass);
  const uint32_t width = std::min<uint32_t>(kPlanTeamsMax, f.grid / T);
  if (width < 2) return 1;
  *team_wgs = T;
  return width;
}

inline AlignPlan plan_align(const AlignFacts& f) {
  if (f.robust || f.prior) {
    // The robust round and the pose prior have instantiations of the single-device launch and of the loop only: an
    // upload never takes the fused launch (it uploads, then plans as a Resident call), a batch is k single aligns.
    AlignFacts g = f;
    g.robust = false;
    g.prior = false;
    g.no_fused = true;
    g.k = 1;
    return plan_align(g);
  }
  AlignPlan p;
  const bool loop_asked = f.profile || f.no_persistent || f.max_iteration <= 0;
  if (f.call == AlignCall::Group) {
    // without the persistent kernel on EVERY device the host-summed loop is the path, not a fallback
    const bool single = f.mailboxes && f.persistent_enabled && !loop_asked && f.cooldown == 0;
    if (f.cooldown > 0 && !loop_asked) p.cooldown_drop = 1;
    p.path = single ? AlignPath::Persistent : AlignPath::GroupLoop;
    return p;
  }
  // the fused launch: only where the single launch would run the one-point-per-thread body on one device
  if (f.call == AlignCall::Upload && f.buffers && f.upload_staged && !loop_asked && !f.no_fused && !f.stamps &&
      !f.stage_events && !f.owner && f.world_size == 1 && !(f.peers_connected && f.peer_world > 1) && f.persistent_enabled &&
      f.cooldown == 0 && f.n > 0 && one_point_per_thread(f.n, f.grid)) {
    p.path = AlignPath::Fused;
    return p;
  }
  if (f.call == AlignCall::Batch) {
    uint32_t T = 0;
    const uint32_t width = team_width(f, &T);
    if (f.k >= 2 && width >= 2 && !loop_asked && f.max_iteration < kBatchSlotRows) {
      p.width = width;
      p.team_wgs = T;
      // inside the cool-down no launch is attempted and nothing is counted: k aligns on the loop, k aligns of cool-down
      p.path = f.cooldown > 0 ? AlignPath::Loop : AlignPath::Teams;
      p.cooldown_drop = std::min<int>(f.cooldown, (int)f.k);
      return p;
    }
  }
  // a single align of the resident scan
  p.peer_path = f.peers_connected && f.peer_enabled && f.peer_world > 1;
  const bool alone = f.world_size == 1;  // also a communicator of one rank: nothing to exchange
  const bool single = !(f.cooldown > 0 && !p.peer_path) && f.persistent_enabled && (alone || p.peer_path) && !loop_asked;
  const bool to_group = f.owner && f.peer_world > 1 && !single;   // a sub-context that does not get the single launch
  // every other align that finds a cool-down off the peer path takes one off it, one that asked for the loop by flag included
  if (f.cooldown > 0 && !p.peer_path && !to_group) p.cooldown_drop = 1;
  p.path = to_group ? AlignPath::GroupLoop : single ? AlignPath::Persistent : AlignPath::Loop;
  return p;
}

}  // namespace vgicp
