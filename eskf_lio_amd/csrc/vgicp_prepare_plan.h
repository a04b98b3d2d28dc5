// vgicp_prepare_plan.h — how a scan preparation's raw sweep reaches the device: ONE pure function of plain facts (no HIP
// call, no context), so that a CPU program can enumerate it (tests/native/prepare_plan.cpp).  DESIGN.md §4 has the table
// written from it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vgicp {

constexpr uint32_t kPlanDeskewMaxStates = 4096;   // vgicp_device.h's kDeskewMaxStates (asserted in vgicp_context.h)
constexpr size_t kPrepareStageLimit = 16u << 20;  // sweeps up to this many bytes are staged (VGICP_STAGE_LIMIT overrides)

enum class PrepareRoute {
  Ahead,    // the sweep lies in a page-locked slot already (vgicp_sweep_stage): nothing is copied by the host
  Staged,   // the copy crew moves it into the pinned raw-sweep slot, the prologue reads the units as they are published
  InPlace   // the runtime copies it out of the caller's memory; waited for before the call returns
};
// where the deskew's first kernel reads the capture times: nowhere (no deskew), the ahead slot, the raw-sweep slot, d_time
enum class TimeSource { None, Ahead, Staged, Device };
// the copy command that brings the capture times to d_time: none, or out of the ahead slot, the raw-sweep slot (this
// thread staged them first), the caller's array
enum class TimeCopy { None, FromAhead, FromStaged, FromCaller };
// where the state-table slot's event is recorded: in enqueue_prepare behind the kernels that read the raw-sweep slot (it
// guards that too), behind enqueue_prepare, or before it and waited for (the caller's buffers are free again on return)
enum class StateTableEvent { Inside, After, BeforeAndWait };

struct PrepareFacts {
  size_t n = 0;
  bool with_deskew = false;
  size_t used = 0;              // states that can own points (deskew_table)
  bool ordered = false;         // their times are finite and non-decreasing
  bool ahead = false;           // the sweep was staged on arrival
  size_t stage_limit = kPrepareStageLimit;
  bool bounds_fused = false;    // prepare_bounds_fused(n, used, ordered): the prologue finds the deskew's segments itself
};

struct PreparePlan {
  PrepareRoute route = PrepareRoute::InPlace;
  bool walk = false;            // the serial bounds walk: reads the times many times over, so they go to device memory
  bool times_by_unit = false;   // the crew stages a unit's capture times with its points
  bool times_by_owner = false;  // the calling thread stages all capture times first, before it joins the crew
  TimeSource time_source = TimeSource::None;
  TimeCopy time_copy = TimeCopy::None;
  StateTableEvent event = StateTableEvent::BeforeAndWait;
};

inline PreparePlan plan_prepare(const PrepareFacts& f) {
  PreparePlan p;
  const size_t raw_bytes = f.n * 3 * sizeof(double) + (f.with_deskew ? f.n * sizeof(double) : 0);
  p.route = f.ahead ? PrepareRoute::Ahead : raw_bytes <= f.stage_limit ? PrepareRoute::Staged : PrepareRoute::InPlace;
  p.walk = f.with_deskew && !(f.ordered && f.used <= kPlanDeskewMaxStates);
  p.event = p.route == PrepareRoute::Ahead ? StateTableEvent::After
          : p.route == PrepareRoute::Staged ? StateTableEvent::Inside : StateTableEvent::BeforeAndWait;
  if (!f.with_deskew) return p;
  if (p.route == PrepareRoute::InPlace) {
    p.time_source = TimeSource::Device;
    p.time_copy = TimeCopy::FromCaller;
    return p;
  }
  // page-locked times: read where they lie, unless the walk wants them on the device
  const bool ahead = p.route == PrepareRoute::Ahead;
  p.time_source = p.walk ? TimeSource::Device : ahead ? TimeSource::Ahead : TimeSource::Staged;
  if (p.walk) p.time_copy = ahead ? TimeCopy::FromAhead : TimeCopy::FromStaged;
  p.times_by_unit = !ahead && !p.walk && f.bounds_fused;
  p.times_by_owner = !ahead && !p.times_by_unit;
  return p;
}

}  // namespace vgicp
