// UpdatePlan.hpp — what ONE LocalMap::updateLocalMap does, decided in one place from the facts of the frame (DESIGN.md
// §9, "Which route an update takes").  Plain data and a pure function: no C ABI, no Eigen, nothing of the class —
// tests/native/update_plan.cpp enumerates every combination of the facts.
#ifndef ESKF_LIO_SHIM_UPDATE_PLAN_HPP_
#define ESKF_LIO_SHIM_UPDATE_PLAN_HPP_

namespace ESKF_LIO
{
namespace shim
{
struct UpdateFacts
{
  // the map (LocalMapConfig as the constructor normalised it, and what became of the shadow grid so far)
  bool deviceResident = false, keepRawPoints = false, rawOnDevice = false, shadowComplete = true;
  // the cloud: it still is the resident scan (asked only with deviceResident: it costs a hash over the cloud), and then
  // whether its host buffers hold the prepared scan (false: the raw sweep, HostCopy::Deferred)
  bool resident = false, hostIsCurrent = false;
  bool initialize = false, hasPrevTransform = false;
  bool moved = false;         // needsMapUpdate(transform); asked only where it decides (insertionDue below)
  bool evictionDue = false;   // removeDistantPoints and the period is over; the clock is read only when insertionDue
  bool soleOwner = false;     // the caller moved its only pointer in (src/Odometry.cpp:86): nobody else can see the cloud
  // LocalMap::setInsertGate(g > 0) on a device-resident map (include/vgicp_hip_map_gated.h).  false: every field of the
  // plan is what it was before the gate existed.  A gated map that keeps raw points keeps them on the device
  // (setInsertGate sees to rawOnDevice, or refuses), so a gated map never has a shadow grid to feed: the gate decides the
  // entry and the count below, nothing else
  bool gated = false;
  // LocalMap::setCarve on a device-resident map (include/vgicp_hip_map_carve.h).  false: every field of the plan is what
  // it is without it.  Like a gated map, a carving map that keeps raw points keeps them on the device (setCarve sees to
  // rawOnDevice, or refuses): the shadow grid is never fed a map it cannot follow
  bool carve = false;
};

struct UpdatePlan
{
  // ResidentScan: the device inserts the scan it already holds.  HostCloud: the device map is fed the host cloud.
  // HostMap: the host grid is authoritative, the device mirror gets the touched and the erased voxels.
  enum class Route {ResidentScan, HostCloud, HostMap};
  enum class Transform {None, Here, OnWorker};        // where the host cloud moves into the world frame
  enum class HandOver {None, MoveCloud, CopyCloud};   // what the shadow grid's worker gets
  Route route = Route::HostMap;
  bool insert = false, evict = false;
  Transform transform = Transform::Here;
  HandOver handOver = HandOver::None;
  bool shadowComplete = true;   // every frame inserted on the device so far has also reached the shadow grid
  // With a gate.  The resident-scan route inserts through vgicp_map_insert_resident_gated_async; a host cloud is no
  // resident scan, so it is inserted whole and the frame is counted (LocalMap::gatedTotals().plainFrames).
  enum class Entry {Plain, Gated};
  Entry entry = Entry::Plain;
  bool countPlain = false;
  // With setCarve.  The resident-scan route carves the map with the scan it is about to insert, at the frame's pose and
  // BEFORE the insertion (vgicp_map_carve_resident_async: enqueued only).  A host cloud is no resident scan, so it casts no
  // rays; the host-authoritative map is never carved.
  bool carve = false;
};

// reference: src/LocalMap.cpp:39 (with prevTransform_ initialised: the first update always inserts)
inline bool insertionDue(const UpdateFacts & f) {return f.initialize || !f.hasPrevTransform || f.moved;}

inline UpdatePlan planUpdate(const UpdateFacts & f)
{
  using Route = UpdatePlan::Route;
  using Transform = UpdatePlan::Transform;
  using HandOver = UpdatePlan::HandOver;
  UpdatePlan p;
  p.route = !f.deviceResident ? Route::HostMap : f.resident ? Route::ResidentScan : Route::HostCloud;
  p.insert = insertionDue(f);
  p.evict = p.insert && f.evictionDue;
  // The host side of an update on the device, for save(): the worker files the cloud's points in the shadow grid.  The
  // resident route hands over every cloud whose host buffers are current (the worker moves a cloud nobody else can see
  // into the world frame even when nothing is inserted); a host cloud was transformed here already and goes over only
  // when it was inserted.
  const bool gated = f.gated && f.deviceResident;   // (a host-authoritative map has no resident route: no gate)
  p.entry = gated && p.route == Route::ResidentScan ? UpdatePlan::Entry::Gated : UpdatePlan::Entry::Plain;
  p.countPlain = gated && p.route == Route::HostCloud && p.insert;
  p.carve = f.carve && f.deviceResident && p.route == Route::ResidentScan && p.insert;
  const bool shadow = f.deviceResident && f.keepRawPoints && !f.rawOnDevice && f.shadowComplete;
  const bool wanted = p.route == Route::ResidentScan ? f.hostIsCurrent : p.route == Route::HostCloud && p.insert;
  // the worker reads the cloud later: it gets the caller's object only when nobody else can reach it, else a copy — a
  // caller that keeps its pointer may edit or resize the cloud as soon as the call returns
  p.handOver = !(shadow && wanted) ? HandOver::None : f.soleOwner ? HandOver::MoveCloud : HandOver::CopyCloud;
  if (p.route != Route::ResidentScan) {
    p.transform = Transform::Here;        // in place, as src/LocalMap.cpp:15, before the insertion reads the cloud
  } else if (!f.hostIsCurrent) {
    p.transform = Transform::None;        // the host holds the raw sweep: nothing of the prepared scan to move
  } else {
    p.transform = p.handOver == HandOver::MoveCloud ? Transform::OnWorker : Transform::Here;
  }
  // an insertion on the resident scan whose points never reach the host: save() falls back to the voxels' means
  p.shadowComplete = f.shadowComplete && !(p.route == Route::ResidentScan && p.insert && p.handOver == HandOver::None);
  return p;
}
}  // namespace shim
}  // namespace ESKF_LIO

#endif  // ESKF_LIO_SHIM_UPDATE_PLAN_HPP_
