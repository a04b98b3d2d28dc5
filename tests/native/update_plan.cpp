// CPU check of shim::planUpdate (include/eskf_lio_shim/UpdatePlan.hpp) alone: every combination of the eleven boolean
// facts of a LocalMap::updateLocalMap, and for each the invariants the routes had when they were written out one after
// the other.  The header needs neither the C ABI nor the boundary types, so nothing else is included or linked.
#include <cstdio>

#include "eskf_lio_shim/UpdatePlan.hpp"

using ESKF_LIO::shim::UpdateFacts;
using ESKF_LIO::shim::UpdatePlan;
using Route = UpdatePlan::Route;
using Transform = UpdatePlan::Transform;
using HandOver = UpdatePlan::HandOver;

static int failures = 0;
static unsigned current = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) { if (++failures <= 20) std::printf("FAILED facts %#x line %d: %s\n", current, __LINE__, #cond); } \
  } while (0)

int main() {
  unsigned seen[3] = {0, 0, 0}, moves = 0, copies = 0, lost = 0;
  for (unsigned bits = 0; bits < (1u << 11); ++bits) {
    current = bits;
    UpdateFacts f;
    f.deviceResident = bits & 1u;
    f.keepRawPoints = bits & 2u;
    f.rawOnDevice = bits & 4u;
    f.shadowComplete = bits & 8u;
    f.resident = bits & 16u;
    f.hostIsCurrent = bits & 32u;
    f.initialize = bits & 64u;
    f.hasPrevTransform = bits & 128u;
    f.moved = bits & 256u;
    f.evictionDue = bits & 512u;
    f.soleOwner = bits & 1024u;
    // what the class never produces: raw points on the device without deviceResident and keepRawPoints (the constructor
    // normalises it), a resident cloud without deviceResident (not asked), a current host without a stamp
    if (f.rawOnDevice && !(f.deviceResident && f.keepRawPoints)) continue;
    if (f.resident && !f.deviceResident) continue;
    if (f.hostIsCurrent && !f.resident) continue;
    const UpdatePlan p = ESKF_LIO::shim::planUpdate(f);
    ++seen[static_cast<int>(p.route)];

    // insert <=> initialize || !hasPrev || moved; evict => insert, and an eviction that is due happens with the insertion
    CHECK(p.insert == (f.initialize || !f.hasPrevTransform || f.moved));
    CHECK(!p.evict || p.insert);
    CHECK(p.evict == (p.insert && f.evictionDue));
    // the routes
    CHECK((p.route == Route::HostMap) == !f.deviceResident);
    CHECK((p.route == Route::ResidentScan) == (f.deviceResident && f.resident));
    // no shadow hand-over with the raw points on the device, without raw points, or once the shadow has lost a frame;
    // none for the host-authoritative map
    if (f.rawOnDevice || !f.keepRawPoints || !f.shadowComplete || !f.deviceResident) CHECK(p.handOver == HandOver::None);
    // with a shadow: every current host cloud of the resident route, every INSERTED cloud of the host-cloud route
    if (f.deviceResident && f.keepRawPoints && !f.rawOnDevice && f.shadowComplete) {
      if (p.route == Route::ResidentScan) CHECK((p.handOver != HandOver::None) == f.hostIsCurrent);
      if (p.route == Route::HostCloud) CHECK((p.handOver != HandOver::None) == p.insert);
    }
    // moved, not copied, only for a sole owner; a sole owner's cloud is never copied
    if (p.handOver == HandOver::MoveCloud) CHECK(f.soleOwner);
    if (p.handOver == HandOver::CopyCloud) CHECK(!f.soleOwner);
    // where the host cloud is transformed: a host cloud always here (the insertion reads it); the resident route's only
    // when the host holds the prepared scan, and on the worker exactly when the worker got the caller's own cloud
    if (p.route != Route::ResidentScan) CHECK(p.transform == Transform::Here);
    if (p.route == Route::ResidentScan && !f.hostIsCurrent) CHECK(p.transform == Transform::None);
    if (p.route == Route::ResidentScan && f.hostIsCurrent) CHECK(p.transform != Transform::None);
    CHECK((p.transform == Transform::OnWorker) == (p.route == Route::ResidentScan && p.handOver == HandOver::MoveCloud));
    // shadowComplete is lost exactly when an insertion happens on the resident route without a hand-over, never regained
    const bool loses = p.route == Route::ResidentScan && p.insert && p.handOver == HandOver::None;
    CHECK(p.shadowComplete == (f.shadowComplete && !loses));
    moves += p.handOver == HandOver::MoveCloud;
    copies += p.handOver == HandOver::CopyCloud;
    lost += f.shadowComplete && !p.shadowComplete;
  }
  // every route, both hand-overs and the loss of the shadow were met
  CHECK(seen[0] && seen[1] && seen[2] && moves && copies && lost);
  if (failures == 0) std::printf("ok %u + %u + %u plans\n", seen[0], seen[1], seen[2]);
  return failures == 0 ? 0 : 1;
}
