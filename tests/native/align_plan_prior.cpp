// The host path of an align while a pose prior is set (AlignFacts::prior, include/vgicp_hip_prior.h), enumerated on the
// CPU over the facts tests/native/align_plan_robust.cpp enumerates: the prior is planned exactly as the robust round is,
// so for every combination the plan with prior = true is the plan of the same facts with robust = true instead — the
// same path, peer path, width, team size and cool-down — and so is the plan with both set; team_width says 1.
// EVERY combination of the boolean facts, the same values for the numeric ones, every kind of call; nothing skipped.
#include <cstdint>
#include <cstdio>

#include "vgicp_align_plan.h"

using namespace vgicp;

static unsigned long long visited = 0, per_path[5] = {0, 0, 0, 0, 0};

static int mismatch(const AlignFacts& f, const AlignPlan& p, const AlignPlan& q, const char* what) {
  std::printf("MISMATCH (%s): call %d n %llu k %zu max_iteration %d profile %d no_persistent %d buffers %d staged %d | persistent %d "
              "owner %d comm %d peers %d peer_enabled %d stamps %d stage_events %d no_fused %d mailboxes %d world %d peer_world %d "
              "cooldown %d grid %u -> prior: path %d peer_path %d drop %d width %u team_wgs %u | robust: path %d peer_path %d "
              "drop %d width %u team_wgs %u\n", what, (int)f.call, (unsigned long long)f.n, f.k, f.max_iteration, f.profile,
              f.no_persistent, f.buffers, f.upload_staged, f.persistent_enabled, f.owner, f.comm, f.peers_connected, f.peer_enabled,
              f.stamps, f.stage_events, f.no_fused, f.mailboxes, f.world_size, f.peer_world, f.cooldown, f.grid, (int)p.path,
              p.peer_path, p.cooldown_drop, p.width, p.team_wgs, (int)q.path, q.peer_path, q.cooldown_drop, q.width, q.team_wgs);
  return 1;
}

static int check(const AlignFacts& f) {
  const AlignPlan p = plan_align(f);
  ++visited;
  ++per_path[(int)p.path];
  AlignFacts robust = f;
  robust.prior = false;
  robust.robust = true;
  const AlignPlan q = plan_align(robust);
  AlignFacts both = f;
  both.robust = true;
  const AlignPlan b = plan_align(both);
  if (p.path == AlignPath::Fused) return mismatch(f, p, q, "fused");
  if (p.path == AlignPath::Teams) return mismatch(f, p, q, "teams");
  uint32_t team_wgs = 7;
  if (team_width(f, &team_wgs) != 1 || team_wgs != 0) return mismatch(f, p, q, "team width");
  if (p.path != q.path || b.path != q.path) return mismatch(f, p, q, "path");
  if (p.peer_path != q.peer_path || b.peer_path != q.peer_path) return mismatch(f, p, q, "peer path");
  if (p.cooldown_drop != q.cooldown_drop || b.cooldown_drop != q.cooldown_drop) return mismatch(f, p, q, "cool-down");
  if (p.width != q.width || p.team_wgs != q.team_wgs || b.width != q.width || b.team_wgs != q.team_wgs) return mismatch(f, p, q, "width");
  return 0;
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
                    f.prior = true;
                    bool* const flags[kBools] = {&f.profile, &f.no_persistent, &f.buffers, &f.upload_staged, &f.persistent_enabled,
                                                 &f.owner, &f.comm, &f.peers_connected, &f.peer_enabled, &f.stamps,
                                                 &f.stage_events, &f.no_fused, &f.mailboxes};
                    for (int b = 0; b < kBools; ++b) *flags[b] = (bits >> b) & 1u;
                    if (check(f)) return 1;
                  }
    }
  const unsigned long long expected = 4ull * 3 * 6 * 3 * 4 * 3 * 2 * 2 * (1ull << kBools);
  if (visited != expected) { std::printf("visited %llu combinations, expected %llu\n", visited, expected); return 1; }
  if (per_path[(int)AlignPath::Fused] != 0 || per_path[(int)AlignPath::Teams] != 0) { std::printf("a fused or team launch was planned\n"); return 1; }
  if (per_path[(int)AlignPath::Persistent] == 0 || per_path[(int)AlignPath::Loop] == 0 || per_path[(int)AlignPath::GroupLoop] == 0) {
    std::printf("a path of the pose prior is never planned\n");
    return 1;
  }
  std::printf("ok %llu combinations: fused %llu persistent %llu teams %llu loop %llu group-loop %llu\n", visited, per_path[0],
              per_path[1], per_path[2], per_path[3], per_path[4]);
  return 0;
}
