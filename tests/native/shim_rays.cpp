// The shim's ray report (include/eskf_lio_shim/LocalMap.hpp: LocalMap::rayReport / rayCounts over
// include/vgicp_hip_map_rays.h) on the CPU, against a stand-in of the C ABI: what the two calls hand to
// vgicp_rays_resident, what they make of its answer, and that a map or a scan that is not on the device gives
// available == false without a throw.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "eskf_lio_shim/LocalMap.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// ---- the C ABI, stubbed ----
struct vgicp_ctx { int unused; };
static vgicp_ctx g_ctx;
static size_t g_scan = 0;          // points of the resident scan
static bool g_scan_resident = false;
static int g_rays_rc = VGICP_OK;
static int g_rays_calls = 0;
static size_t g_last_poses = 0;
static double g_last_pose0[16];
static vgicp_ray_params g_last_params;
static bool g_last_per_point = false;
extern "C" {
int vgicp_create(int, vgicp_ctx** out) { *out = &g_ctx; return VGICP_OK; }
int vgicp_create_multi(const int*, int, vgicp_ctx** out) { *out = &g_ctx; return VGICP_OK; }
int vgicp_destroy(vgicp_ctx*) { return VGICP_OK; }
const char* vgicp_last_error(const vgicp_ctx*) { return "stub"; }
int vgicp_map_reset(vgicp_ctx*, double, size_t) { return VGICP_OK; }
int vgicp_map_upsert(vgicp_ctx*, size_t, const int32_t*, const double*, const double*) { return VGICP_OK; }
int vgicp_map_erase(vgicp_ctx*, size_t, const int32_t*) { return VGICP_OK; }
int vgicp_map_size(const vgicp_ctx*, size_t* voxels, size_t* slots) { if (voxels) *voxels = 0; if (slots) *slots = 0; return VGICP_OK; }
int vgicp_map_export(vgicp_ctx*, size_t, int32_t*, double*, double*, uint64_t*, size_t* written) { if (written) *written = 0; return VGICP_OK; }
int vgicp_map_insert_scan(vgicp_ctx*, size_t, const double*, const double*, const double*, size_t, size_t* new_voxels) { if (new_voxels) *new_voxels = 0; return VGICP_OK; }
int vgicp_map_insert_resident_async(vgicp_ctx*, const double*, size_t) { return VGICP_OK; }
int vgicp_map_evict(vgicp_ctx*, const double*, double, size_t* removed) { if (removed) *removed = 0; return VGICP_OK; }
int vgicp_match(vgicp_ctx*, size_t, const double*, const double*, double*, double*, double*, double*, uint64_t*, size_t* matched) { if (matched) *matched = 0; return VGICP_OK; }
int vgicp_get_counter(const vgicp_ctx*, int, uint64_t* value) { if (value) *value = 0; return VGICP_OK; }
int vgicp_scan_download(vgicp_ctx*, size_t, double*, double*, size_t* n) {
  if (n) *n = g_scan_resident ? g_scan : 0;
  return g_scan_resident ? VGICP_OK : VGICP_ERR_NOT_READY;
}
int vgicp_rays_resident(vgicp_ctx*, const double* poses, size_t n_poses, const vgicp_ray_params* params,
                        const vgicp_ray_outputs* per_point, vgicp_ray_counts* counts, vgicp_ray_stats*) {
  ++g_rays_calls;
  if (!g_scan_resident) return VGICP_ERR_NOT_READY;
  if (g_rays_rc != VGICP_OK) return g_rays_rc;
  g_last_poses = n_poses;
  std::memcpy(g_last_pose0, poses, sizeof g_last_pose0);
  g_last_params = *params;
  g_last_per_point = per_point != nullptr;
  for (size_t k = 0; k < n_poses; ++k) {
    counts[k].rays = 100 + k;
    counts[k].visits = 1000 + k;
    for (int c = 0; c < 8; ++c) counts[k].by_class[c] = 10 * k + c;
  }
  if (per_point) {
    for (size_t i = 0; i < g_scan; ++i) {
      per_point->status[i] = (uint8_t)(i % 7);
      per_point->range[i] = 0.5 * (double)i;
      for (int a = 0; a < 3; ++a) per_point->hit_key[3 * i + a] = (int32_t)(3 * i + a);
      per_point->steps[i] = (uint32_t)(i + 1);
    }
  }
  return VGICP_OK;
}
}

int main() {
  using namespace ESKF_LIO;
  LocalMapConfig onDevice;
  LocalMapConfig onHost = onDevice;
  onHost.deviceResident = false;
  LocalMap map(onDevice, false, &g_ctx), hostMap(onHost, false, &g_ctx);
  Isometry3d T = Isometry3d::Identity();
  T.matrix()(0, 3) = 1.5;
  T.matrix()(2, 3) = -0.25;
  const LocalMap::RayParams params = {{0.1, 0.2, 0.3}, 1.0, 20.0, 60.0, 3, 0};

  // no resident scan: not available, nothing thrown
  LocalMap::RayReport none = map.rayReport(T, params);
  CHECK(!none.available && none.status.empty() && none.range.empty() && none.hitKey.empty() && none.steps.empty());
  CHECK(none.counts.rays == 0 && none.counts.visits == 0);
  LocalMap::RayCountsList noCounts = map.rayCounts({T, T}, params);
  CHECK(!noCounts.available && noCounts.counts.empty());

  // a host-authoritative map never asks the device
  g_scan_resident = true;
  g_scan = 9;
  const int calls = g_rays_calls;
  CHECK(!hostMap.rayReport(T, params).available && !hostMap.rayCounts({T}, params).available && g_rays_calls == calls);

  // the report: one pose, the planes of the scan's size, the counts
  LocalMap::RayReport r = map.rayReport(T, params);
  CHECK(r.available && g_last_poses == 1 && g_last_per_point);
  CHECK(std::memcmp(g_last_pose0, T.matrix().data(), sizeof g_last_pose0) == 0);
  CHECK(std::memcmp(&g_last_params, &params, sizeof params) == 0);
  CHECK(r.status.size() == 9 && r.range.size() == 9 && r.hitKey.size() == 27 && r.steps.size() == 9);
  CHECK(r.status[8] == 1 && r.range[8] == 4.0 && r.hitKey[26] == 26 && r.steps[8] == 9);
  CHECK(r.counts.rays == 100 && r.counts.visits == 1000 && r.counts.byClass[VGICP_RAY_BLOCKED] == 5);

  // the counts at several poses: no planes asked for
  Isometry3d U = T;
  U.matrix()(1, 3) = 7.0;
  LocalMap::RayCountsList c = map.rayCounts({U, T, T}, params);
  CHECK(c.available && c.counts.size() == 3 && g_last_poses == 3 && !g_last_per_point);
  CHECK(std::memcmp(g_last_pose0, U.matrix().data(), sizeof g_last_pose0) == 0);
  CHECK(c.counts[2].rays == 102 && c.counts[2].visits == 1002 && c.counts[2].byClass[VGICP_RAY_BEHIND] == 23);
  CHECK(!map.rayCounts({}, params).available);

  // a refusal of the arguments is an error, as everywhere in the shim
  g_rays_rc = VGICP_ERR_BAD_ARGUMENT;
  bool threw = false;
  try {
    (void)map.rayReport(T, params);
  } catch (const std::exception &) {
    threw = true;
  }
  CHECK(threw);
  // ... and a scan that went away between the size query and the call is "not available"
  g_rays_rc = VGICP_ERR_NOT_READY;
  CHECK(!map.rayReport(T, params).available && !map.rayCounts({T}, params).available);
  std::printf("ok\n");
  return 0;
}
