// How a scan preparation's raw sweep reaches the device (eskf_lio_amd/csrc/vgicp_prepare_plan.h: plan_prepare), enumerated
// on the CPU against the predicates scan_prepare_enqueue spelled out by hand before they became one function — copied
// here as they stood (`staged`, `walk`, `times_by_unit`, `time_src`, `dk.point_time`, the three sites of the state-table
// slot's event, the final wait), with the pointers replaced by tags and every runtime call by a note of what it did.
// EVERY combination of the facts' values below; nothing skipped.
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "vgicp_prepare_plan.h"

using namespace vgicp;

namespace old {
constexpr uint32_t kDeskewMaxStates = 4096;
// the arrays a capture time can be read from / copied out of
enum Where { kNowhere, kAheadSlot, kStagedTimes, kCallerTimes, kDeviceTimes };

struct Enqueue {
  bool staged = false, walk = false, times_by_unit = false;
  bool crew_posted = false;          // post_sweep_copy
  bool owner_staged_times = false;   // stage_copy(times_stage, point_time, ...) on the calling thread
  bool points_copy_command = false;  // hipMemcpyAsync(d_pts, points, ...)
  Where time_copy_from = kNowhere;   // hipMemcpyAsync(d_time, <this>, ...)
  Where point_time = kNowhere;       // dk.point_time
  bool event_before = false, event_wait = false, event_inside = false, event_after = false;
  bool sp_given = false;             // enqueue_prepare(..., staged ? &sp : nullptr)
  bool sp_points = false;            // sp.points != nullptr: the crew's branch of enqueue_prepare
};

Enqueue scan_prepare_enqueue(size_t n, bool with_deskew, size_t used, bool ordered, bool ahead, size_t stage_limit,
                             bool bounds_fused) {
  Enqueue e;
  const size_t raw_bytes = n * 3 * sizeof(double) + (with_deskew ? n * sizeof(double) : 0);
  const bool staged = ahead || raw_bytes <= stage_limit;   // larger sweeps go up straight from the caller's memory
  const bool walk = with_deskew && !(ordered && used <= kDeskewMaxStates);   // the serial bounds walk reads the times many times over: on the device
  Where time_src = kNowhere;   // where the deskew's first kernel reads the capture times
  const Where point_time = ahead ? kAheadSlot : kCallerTimes, times_stage = kStagedTimes, d_time = kDeviceTimes;
  if (ahead) {
    if (with_deskew) {
      time_src = point_time;
      if (walk) e.time_copy_from = point_time;
    }
  } else if (staged) {
    e.sp_points = true;
    e.event_inside = true;   // sp.done = ctx->ev_state_table[slot], recorded by enqueue_prepare
    const bool times_by_unit = with_deskew && !walk && bounds_fused;
    e.times_by_unit = times_by_unit;
    e.crew_posted = true;
    if (times_by_unit) {
      time_src = times_stage;
    } else if (with_deskew) {
      e.owner_staged_times = true;
      time_src = times_stage;
      if (walk) e.time_copy_from = times_stage;
    }
  } else {
    e.points_copy_command = true;
    if (with_deskew) e.time_copy_from = point_time;
  }
  if (with_deskew) e.point_time = (staged && !walk) ? time_src : d_time;
  if (!staged) {
    e.event_before = true;
    e.event_wait = true;
  }
  e.sp_given = staged;
  if (ahead) e.event_after = true;
  e.staged = staged;
  e.walk = walk;
  return e;
}
}  // namespace old

static unsigned long long visited = 0, per_route[3] = {0, 0, 0}, per_source[4] = {0, 0, 0, 0};

static int mismatch(const PrepareFacts& f, const PreparePlan& p, const char* what) {
  std::printf("MISMATCH (%s): n %zu with_deskew %d used %zu ordered %d ahead %d stage_limit %zu bounds_fused %d -> route %d walk %d "
              "times_by_unit %d times_by_owner %d time_source %d time_copy %d event %d\n", what, f.n, f.with_deskew, f.used,
              f.ordered, f.ahead, f.stage_limit, f.bounds_fused, (int)p.route, p.walk, p.times_by_unit, p.times_by_owner,
              (int)p.time_source, (int)p.time_copy, (int)p.event);
  return 1;
}

static int check(const PrepareFacts& f) {
  const PreparePlan p = plan_prepare(f);
  const old::Enqueue e = old::scan_prepare_enqueue(f.n, f.with_deskew, f.used, f.ordered, f.ahead, f.stage_limit, f.bounds_fused);
  ++visited;
  ++per_route[(int)p.route];
  ++per_source[(int)p.time_source];
  // the route: which branch staged the sweep, and which branch of enqueue_prepare it takes
  const PrepareRoute route = f.ahead ? PrepareRoute::Ahead : e.staged ? PrepareRoute::Staged : PrepareRoute::InPlace;
  if (p.route != route) return mismatch(f, p, "route");
  if ((p.route != PrepareRoute::InPlace) != e.sp_given || (p.route == PrepareRoute::Staged) != e.sp_points ||
      (p.route == PrepareRoute::Staged) != e.crew_posted || (p.route == PrepareRoute::InPlace) != e.points_copy_command)
    return mismatch(f, p, "what the route does");
  if (p.walk != e.walk) return mismatch(f, p, "walk");
  if (p.times_by_unit != e.times_by_unit) return mismatch(f, p, "times by unit");
  if (p.times_by_owner != e.owner_staged_times) return mismatch(f, p, "times by the calling thread");
  // the deskew's first kernel
  const old::Where source[] = {old::kNowhere, old::kAheadSlot, old::kStagedTimes, old::kDeviceTimes};
  if (source[(int)p.time_source] != e.point_time) return mismatch(f, p, "time source");
  const old::Where copy_from[] = {old::kNowhere, old::kAheadSlot, old::kStagedTimes, old::kCallerTimes};
  if (copy_from[(int)p.time_copy] != e.time_copy_from) return mismatch(f, p, "time copy");
  // the state-table slot's event, and the wait that ends the in-place route
  const bool inside = p.event == StateTableEvent::Inside, after = p.event == StateTableEvent::After,
             before = p.event == StateTableEvent::BeforeAndWait;
  if (inside != e.event_inside || after != e.event_after || before != e.event_before || before != e.event_wait)
    return mismatch(f, p, "state-table event");
  return 0;
}

int main() {
  const size_t useds[] = {1, 4096, 4097, 16000};
  // n * 32 (points and times) and n * 24 (points) bytes exactly on and one point past the 16 MB default
  const size_t ns[] = {1, 524288, 524289, 699050, 699051};
  const size_t limits[] = {0, 1, (size_t)16 << 20, SIZE_MAX};
  for (uint32_t bits = 0; bits < 16; ++bits)
    for (size_t used : useds)
      for (size_t n : ns)
        for (size_t limit : limits) {
          PrepareFacts f;
          f.ahead = bits & 1u;
          f.with_deskew = (bits >> 1) & 1u;
          f.ordered = (bits >> 2) & 1u;
          f.bounds_fused = (bits >> 3) & 1u;
          f.used = used;
          f.n = n;
          f.stage_limit = limit;
          if (check(f)) return 1;
        }
  const unsigned long long expected = 16ull * 4 * 5 * 4;
  if (visited != expected) { std::printf("visited %llu combinations, expected %llu\n", visited, expected); return 1; }
  for (int r = 0; r < 3; ++r)
    if (per_route[r] == 0) { std::printf("PrepareRoute %d is never planned\n", r); return 1; }
  for (int s = 0; s < 4; ++s)
    if (per_source[s] == 0) { std::printf("TimeSource %d is never planned\n", s); return 1; }
  std::printf("ok %llu combinations: ahead %llu staged %llu in-place %llu | none %llu ahead-slot %llu staged-times %llu device %llu\n",
              visited, per_route[0], per_route[1], per_route[2], per_source[0], per_source[1], per_source[2], per_source[3]);
  return 0;
}
