// CPU check of shim::planUpdate (include/eskf_lio_shim/UpdatePlan.hpp) with LocalMap::setInsertGate: every combination of
// the eleven boolean facts tests/native/update_plan.cpp enumerates, each without and with the gate.
//   gate off   the plan is, field by field, the plan from before the gate existed (restated below as it was written),
//              the entry is the plain one, nothing is counted;
//   gate on    the resident-scan route inserts through the gated entry; a host cloud is inserted plainly and counted; every
//              other field is the former plan's.  A gated map that keeps raw points keeps them on the device
//              (LocalMap::setInsertGate switches the store on or refuses), so those states have no shadow grid and nothing
//              is handed to its worker; the states the class never produces — a gate with raw points kept on the host —
//              are skipped.  A host-authoritative map (no resident route) is planned as without the gate.
#include <cstdio>

#include "eskf_lio_shim/UpdatePlan.hpp"

using ESKF_LIO::shim::UpdateFacts;
using ESKF_LIO::shim::UpdatePlan;
using Route = UpdatePlan::Route;
using Transform = UpdatePlan::Transform;
using HandOver = UpdatePlan::HandOver;
using Entry = UpdatePlan::Entry;

static int failures = 0;
static unsigned current = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) { if (++failures <= 20) std::printf("FAILED facts %#x line %d: %s\n", current, __LINE__, #cond); } \
  } while (0)

// planUpdate as it stood before the gate
static UpdatePlan plan_before(const UpdateFacts & f)
{
  UpdatePlan p;
  p.route = !f.deviceResident ? Route::HostMap : f.resident ? Route::ResidentScan : Route::HostCloud;
  p.insert = f.initialize || !f.hasPrevTransform || f.moved;
  p.evict = p.insert && f.evictionDue;
  const bool shadow = f.deviceResident && f.keepRawPoints && !f.rawOnDevice && f.shadowComplete;
  const bool wanted = p.route == Route::ResidentScan ? f.hostIsCurrent : p.route == Route::HostCloud && p.insert;
  p.handOver = !(shadow && wanted) ? HandOver::None : f.soleOwner ? HandOver::MoveCloud : HandOver::CopyCloud;
  if (p.route != Route::ResidentScan) {
    p.transform = Transform::Here;
  } else if (!f.hostIsCurrent) {
    p.transform = Transform::None;
  } else {
    p.transform = p.handOver == HandOver::MoveCloud ? Transform::OnWorker : Transform::Here;
  }
  p.shadowComplete = f.shadowComplete && !(p.route == Route::ResidentScan && p.insert && p.handOver == HandOver::None);
  return p;
}
static bool same_old_fields(const UpdatePlan & a, const UpdatePlan & b)
{
  return a.route == b.route && a.insert == b.insert && a.evict == b.evict && a.transform == b.transform &&
         a.handOver == b.handOver && a.shadowComplete == b.shadowComplete;
}

int main() {
  unsigned gated_entries = 0, counted = 0, plans = 0;
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
    if (f.rawOnDevice && !(f.deviceResident && f.keepRawPoints)) continue;
    if (f.resident && !f.deviceResident) continue;
    if (f.hostIsCurrent && !f.resident) continue;
    const UpdatePlan before = plan_before(f);
    // gate off: today's plan
    const UpdatePlan off = ESKF_LIO::shim::planUpdate(f);
    CHECK(same_old_fields(off, before));
    CHECK(off.entry == Entry::Plain && !off.countPlain);
    // gate on
    f.gated = true;
    const UpdatePlan on = ESKF_LIO::shim::planUpdate(f);
    if (f.deviceResident && f.keepRawPoints && !f.rawOnDevice) continue;   // setInsertGate never leaves a map so
    ++plans;
    CHECK(same_old_fields(on, before));
    CHECK((on.entry == Entry::Gated) == (f.deviceResident && on.route == Route::ResidentScan));
    CHECK(on.countPlain == (f.deviceResident && on.route == Route::HostCloud && on.insert));
    if (f.deviceResident) CHECK(on.handOver == HandOver::None && on.transform != Transform::OnWorker);
    gated_entries += on.entry == Entry::Gated;
    counted += on.countPlain;
  }
  CHECK(gated_entries && counted);
  if (failures == 0) std::printf("ok %u plans, %u through the gated entry, %u plain frames counted\n", plans, gated_entries, counted);
  return failures == 0 ? 0 : 1;
}
