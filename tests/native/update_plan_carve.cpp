// CPU check of shim::planUpdate (include/eskf_lio_shim/UpdatePlan.hpp) with LocalMap::setCarve: every combination of the
// twelve boolean facts from before (the eleven of tests/native/update_plan.cpp and the gate), each without and with the
// new fact.
//   carve off  the plan is, field by field, the plan the function gives today (restated below as it stands without the
//              new fact), and plan.carve is false;
//   carve on   every former field is unchanged, and plan.carve is set exactly on the resident-scan route of a
//              device-resident map with an insertion due: a host cloud casts no rays, the host-authoritative map is never
//              carved, and a frame that inserts nothing carves nothing.
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

// planUpdate as it stands without the new fact
static UpdatePlan plan_before(const UpdateFacts & f)
{
  UpdatePlan p;
  p.route = !f.deviceResident ? Route::HostMap : f.resident ? Route::ResidentScan : Route::HostCloud;
  p.insert = f.initialize || !f.hasPrevTransform || f.moved;
  p.evict = p.insert && f.evictionDue;
  const bool gated = f.gated && f.deviceResident;
  p.entry = gated && p.route == Route::ResidentScan ? Entry::Gated : Entry::Plain;
  p.countPlain = gated && p.route == Route::HostCloud && p.insert;
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
         a.handOver == b.handOver && a.shadowComplete == b.shadowComplete && a.entry == b.entry && a.countPlain == b.countPlain;
}

int main() {
  unsigned plans = 0, identical = 0, carved = 0;
  if (UpdateFacts().carve) {std::printf("FAILED: UpdateFacts::carve defaults to true\n"); return 1;}
  for (unsigned bits = 0; bits < (1u << 12); ++bits) {
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
    f.gated = bits & 2048u;
    if (f.rawOnDevice && !(f.deviceResident && f.keepRawPoints)) continue;
    if (f.resident && !f.deviceResident) continue;
    if (f.hostIsCurrent && !f.resident) continue;
    if (f.gated && f.deviceResident && f.keepRawPoints && !f.rawOnDevice) continue;   // setInsertGate never leaves a map so
    const UpdatePlan before = plan_before(f);
    // carve off: today's plan
    const UpdatePlan off = ESKF_LIO::shim::planUpdate(f);
    ++plans;
    CHECK(same_old_fields(off, before) && !off.carve);
    identical += same_old_fields(off, before) && !off.carve;
    // carve on (setCarve never leaves a map with its raw points on the host: those states the class does not produce)
    if (f.deviceResident && f.keepRawPoints && !f.rawOnDevice) continue;
    f.carve = true;
    const UpdatePlan on = ESKF_LIO::shim::planUpdate(f);
    ++plans;
    CHECK(same_old_fields(on, before));
    CHECK(on.carve == (f.deviceResident && on.route == Route::ResidentScan && on.insert));
    if (on.carve) CHECK(on.handOver == HandOver::None && on.transform != Transform::OnWorker);   // no shadow grid to feed
    if (on.route != Route::ResidentScan || !on.insert) CHECK(!on.carve);
    carved += on.carve;
  }
  CHECK(carved);
  if (failures == 0) std::printf("ok %u plans, %u identical without carve, %u carve before the insertion\n", plans, identical, carved);
  return failures == 0 ? 0 : 1;
}
