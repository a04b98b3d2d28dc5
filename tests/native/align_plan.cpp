// Which host path an align takes (eskf_lio_amd/csrc/vgicp_align_plan.h: plan_align, team_width, one_point_per_thread),
// enumerated on the CPU against the five predicates the host code spelled out by hand before they became one function
// — copied here as they stood, with `ctx->` / `params->` read from the same facts struct:
//   fused_align_fits (vgicp_align), single_launch + the cool-down step + kNeedGroupLoop (run_align), batch_width + wide
//   + the cool-down branch (vgicp_align_resident_batch), the one-point-per-thread test (wants_dense, persistent_args),
//   single + the group's cool-down step (align_shards).
// EVERY combination of the boolean facts, a handful of values for the numeric ones, every kind of call; nothing skipped.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "vgicp_align_plan.h"

using namespace vgicp;

namespace old {
constexpr int kTeamsMax = 16;
constexpr int kBatchSlotRows = 64;

bool fused_align_fits(const AlignFacts& f) {
  return f.buffers && f.max_iteration > 0 && !(f.profile || f.no_persistent) &&
         !f.no_fused && !f.stamps && !f.stage_events && !f.owner &&
         f.world_size == 1 && !(f.peers_connected && f.peer_world > 1) && f.persistent_enabled &&
         f.cooldown == 0 && f.n > 0 && f.n <= (size_t)f.grid * 448u &&
         f.upload_staged;
}

struct Resident { bool need_group_loop, single_launch, peer_path; int cooldown; };
Resident run_align(const AlignFacts& f) {
  Resident r;
  r.cooldown = f.cooldown;
  const bool loop_only = false;
  const bool profile = f.profile;
  const int max_it = f.max_iteration;
  const bool peer_path = f.peers_connected && f.peer_enabled && f.peer_world > 1;
  const bool alone = f.world_size == 1;
  const bool single_launch = !loop_only && !(f.cooldown > 0 && !peer_path) && f.persistent_enabled &&
                             (alone || peer_path) && !profile && max_it > 0 &&
                             !f.no_persistent;
  r.peer_path = peer_path;
  r.single_launch = single_launch;
  r.need_group_loop = f.owner && f.peer_world > 1 && !single_launch;
  if (r.need_group_loop) return r;
  if (loop_only) {
  } else if (r.cooldown > 0 && !peer_path) --r.cooldown;
  return r;
}

uint32_t batch_width(const AlignFacts& f, uint32_t* team_wgs) {
  *team_wgs = 0;
  const bool one_device = f.world_size == 1 && !f.owner && !f.comm && !f.peers_connected;
  if (!one_device || !f.persistent_enabled || f.stamps || f.n == 0 ||
      (uint64_t)f.n > (uint64_t)f.grid * 448u)
    return 1;
  const uint32_t n = (uint32_t)f.n;
  const uint32_t T = (n + 447u) / 448u;
  const uint32_t width = std::min<uint32_t>((uint32_t)kTeamsMax, f.grid / T);
  if (width < 2) return 1;
  *team_wgs = T;
  return width;
}

struct Group { bool single; int cooldown; };
Group align_shards(const AlignFacts& f) {
  Group g;
  g.cooldown = f.cooldown;
  const bool host_loop_asked = (f.profile || f.no_persistent) || f.max_iteration <= 0;
  const bool all_persistent = f.persistent_enabled;
  g.single = f.mailboxes && all_persistent && !host_loop_asked && g.cooldown == 0;
  if (g.cooldown > 0 && !host_loop_asked) --g.cooldown;
  return g;
}
}  // namespace old

static unsigned long long visited = 0, per_path[5] = {0, 0, 0, 0, 0};

static int mismatch(const AlignFacts& f, const AlignPlan& p, const char* what) {
  std::printf("MISMATCH (%s): call %d n %llu k %zu max_iteration %d profile %d no_persistent %d buffers %d staged %d | persistent %d "
              "owner %d comm %d peers %d peer_enabled %d stamps %d stage_events %d no_fused %d mailboxes %d world %d peer_world %d "
              "cooldown %d grid %u -> path %d peer_path %d drop %d width %u team_wgs %u\n", what, (int)f.call,
              (unsigned long long)f.n, f.k, f.max_iteration, f.profile, f.no_persistent, f.buffers, f.upload_staged,
              f.persistent_enabled, f.owner, f.comm, f.peers_connected, f.peer_enabled, f.stamps, f.stage_events, f.no_fused,
              f.mailboxes, f.world_size, f.peer_world, f.cooldown, f.grid, (int)p.path, p.peer_path, p.cooldown_drop, p.width,
              p.team_wgs);
  return 1;
}

// a single align of the resident scan: also what vgicp_align does after its upload when it is not fused, and what a
// batch does k times when it is not wide
static int check_resident(const AlignFacts& f, const AlignPlan& p) {
  const old::Resident r = old::run_align(f);
  const AlignPath want = r.need_group_loop ? AlignPath::GroupLoop : r.single_launch ? AlignPath::Persistent : AlignPath::Loop;
  if (p.path != want || p.width != 1 || p.team_wgs != 0) return mismatch(f, p, "resident path");
  if (f.cooldown - p.cooldown_drop != r.cooldown) return mismatch(f, p, "resident cool-down");
  if (p.peer_path != r.peer_path) return mismatch(f, p, "peer path");
  return 0;
}

static int check(const AlignFacts& f) {
  const AlignPlan p = plan_align(f);
  ++visited;
  ++per_path[(int)p.path];
  if (one_point_per_thread(f.n, f.grid) != !((uint64_t)f.n > (uint64_t)f.grid * 448u) ||      // wants_dense
      one_point_per_thread(f.n, f.grid) != ((uint32_t)f.n <= f.grid * 448u))                  // persistent_args
    return mismatch(f, p, "one point per thread");
  switch (f.call) {
    case AlignCall::Group: {
      const old::Group g = old::align_shards(f);
      if ((p.path == AlignPath::Persistent) != g.single || (p.path != AlignPath::Persistent && p.path != AlignPath::GroupLoop))
        return mismatch(f, p, "group path");
      if (f.cooldown - p.cooldown_drop != g.cooldown) return mismatch(f, p, "group cool-down");
      return 0;
    }
    case AlignCall::Upload:
      if ((p.path == AlignPath::Fused) != old::fused_align_fits(f)) return mismatch(f, p, "fused");
      if (p.path == AlignPath::Fused) return p.cooldown_drop == 0 && p.width == 1 ? 0 : mismatch(f, p, "fused extras");
      return check_resident(f, p);
    case AlignCall::Batch: {
      uint32_t team_wgs = 0, tw = 0;
      const uint32_t width = old::batch_width(f, &team_wgs);
      if (team_width(f, &tw) != width || tw != team_wgs) return mismatch(f, p, "team width");
      const int max_it = f.max_iteration;
      const bool wide = f.k >= 2 && width >= 2 && max_it > 0 && max_it < old::kBatchSlotRows &&
                        !(f.profile || f.no_persistent);
      if (!wide) return check_resident(f, p);
      if (p.width != width || p.team_wgs != team_wgs) return mismatch(f, p, "wide batch");
      if (f.cooldown > 0) {
        if (p.path != AlignPath::Loop || f.cooldown - p.cooldown_drop != std::max(0, f.cooldown - (int)f.k))
          return mismatch(f, p, "batch inside the cool-down");
      } else if (p.path != AlignPath::Teams || p.cooldown_drop != 0) {
        return mismatch(f, p, "teams");
      }
      return 0;
    }
    case AlignCall::Resident: return check_resident(f, p);
  }
  return mismatch(f, p, "unknown call");
}

int main() {
  const AlignCall calls[] = {AlignCall::Upload, AlignCall::Resident, AlignCall::Batch, AlignCall::Group};
  const uint32_t grids[] = {8, 122, 256};
  const int cooldowns[] = {0, 1, 8}, max_its[] = {0, 1, 63, 64}, worlds[] = {1, 2};
  const size_t ks[] = {1, 2, 16};
  constexpr int kBools = 13;
  for (AlignCall call : calls)
    for (uint32_t grid : grids) {
      const uint64_t ns[] = {0, 1, 448, 449, (uint64_t)grid * 448, (uint64_t)grid * 448 + 1};
      for (uint64_t n : ns)
        for (int cooldown : cooldowns)
          for (int max_it : max_its)
            for (size_t k : ks)
              for (int world : worlds)
                for (int peer_world : worlds)
                  for (uint32_t bits = 0; bits < (1u << kBools); ++bits) {
                    AlignFacts f;
                    f.call = call;
                    f.grid = grid;
                    f.n = n;
                    f.cooldown = cooldown;
                    f.max_iteration = max_it;
                    f.k = k;
                    f.world_size = world;
                    f.peer_world = peer_world;
                    bool* const flags[kBools] = {&f.profile, &f.no_persistent, &f.buffers, &f.upload_staged, &f.persistent_enabled,
                                                 &f.owner, &f.comm, &f.peers_connected, &f.peer_enabled, &f.stamps,
                                                 &f.stage_events, &f.no_fused, &f.mailboxes};
                    for (int b = 0; b < kBools; ++b) *flags[b] = (bits >> b) & 1u;
                    if (check(f)) return 1;
                  }
    }
  const unsigned long long expected = 4ull * 3 * 6 * 3 * 4 * 3 * 2 * 2 * (1ull << kBools);
  if (visited != expected) { std::printf("visited %llu combinations, expected %llu\n", visited, expected); return 1; }
  for (int path = 0; path < 5; ++path)
    if (per_path[path] == 0) { std::printf("AlignPath %d is never planned\n", path); return 1; }
  std::printf("ok %llu combinations: fused %llu persistent %llu teams %llu loop %llu group-loop %llu\n", visited, per_path[0],
              per_path[1], per_path[2], per_path[3], per_path[4]);
  return 0;
}
