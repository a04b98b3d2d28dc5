// The shim's merge member (include/eskf_lio_shim/LocalMap.hpp: LocalMap::mergeFrom over include/vgicp_hip_map_merge.h) on
// the CPU, against a stand-in of the C ABI.  Built twice: as it is, the stand-in has vgicp_map_merge and records what it
// was handed — the two contexts, the frame column-major, the centre, the radius and the two counts — and the modes that
// keep a host shadow grid refuse before the library is asked; with -DWITHOUT_MERGE_LIBRARY the stand-in lacks the entry
// point, as a program linked without libvgicp_hip_map_merge.so does, and mergeFrom throws.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "eskf_lio_shim/Registration.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// ---- the C ABI, stubbed ----
struct vgicp_ctx { int unused; };
static vgicp_ctx g_ctx, g_other;
static std::vector<std::string> g_calls;
static void note(const std::string & s) {g_calls.push_back(s);}
extern "C" {
int vgicp_create(int, vgicp_ctx** out) { *out = &g_ctx; return VGICP_OK; }
int vgicp_create_multi(const int*, int, vgicp_ctx** out) { *out = &g_ctx; return VGICP_OK; }
int vgicp_destroy(vgicp_ctx*) { return VGICP_OK; }
const char* vgicp_last_error(const vgicp_ctx*) { return "stub"; }
int vgicp_map_reset(vgicp_ctx*, double, size_t) { note("map_reset"); return VGICP_OK; }
int vgicp_map_upsert(vgicp_ctx*, size_t, const int32_t*, const double*, const double*) { return VGICP_OK; }
int vgicp_map_erase(vgicp_ctx*, size_t, const int32_t*) { return VGICP_OK; }
int vgicp_map_size(const vgicp_ctx*, size_t* voxels, size_t* slots) { if (voxels) *voxels = 0; if (slots) *slots = 0; return VGICP_OK; }
int vgicp_map_export(vgicp_ctx*, size_t, int32_t*, double*, double*, uint64_t*, size_t* written) { if (written) *written = 0; return VGICP_OK; }
int vgicp_map_insert_scan(vgicp_ctx*, size_t n, const double*, const double*, const double*, size_t, size_t* new_voxels) {
  note("insert_scan " + std::to_string(n));
  if (new_voxels) *new_voxels = 0;
  return VGICP_OK;
}
int vgicp_map_insert_resident_async(vgicp_ctx*, const double*, size_t) { return VGICP_OK; }
int vgicp_map_evict(vgicp_ctx*, const double*, double, size_t* removed) { if (removed) *removed = 0; return VGICP_OK; }
int vgicp_match(vgicp_ctx*, size_t, const double*, const double*, double*, double*, double*, double*, uint64_t*, size_t* matched) { if (matched) *matched = 0; return VGICP_OK; }
int vgicp_get_counter(const vgicp_ctx*, int, uint64_t* value) { if (value) *value = 0; return VGICP_OK; }
int vgicp_scan_download(vgicp_ctx*, size_t, double*, double*, size_t* n) { if (n) *n = 0; return VGICP_ERR_NOT_READY; }
int vgicp_scan_upload(vgicp_ctx*, size_t, const double*, const double*) { return VGICP_OK; }
int vgicp_align(vgicp_ctx*, size_t, const double*, const double*, const double* guess, const vgicp_params*, double* pose, vgicp_stats*) {
  std::memcpy(pose, guess, 16 * sizeof(double));
  return VGICP_OK;
}
int vgicp_align_resident(vgicp_ctx*, const double* guess, const vgicp_params*, double* pose, vgicp_stats*) {
  std::memcpy(pose, guess, 16 * sizeof(double));
  return VGICP_OK;
}
int vgicp_align_resident_batch(vgicp_ctx*, size_t, const double*, const vgicp_params*, double*, vgicp_batch_stats*) { return VGICP_OK; }
int vgicp_align_batch_width(vgicp_ctx*, size_t* w) { if (w) *w = 1; return VGICP_OK; }
int vgicp_evaluate_resident(vgicp_ctx*, size_t, const double*, vgicp_evaluation*, vgicp_eval_stats*) { return VGICP_OK; }
#ifndef WITHOUT_MERGE_LIBRARY
static vgicp_merge_params g_params;
static vgicp_ctx * g_dst = nullptr, * g_src = nullptr;
int vgicp_map_merge(vgicp_ctx* dst, vgicp_ctx* src, const vgicp_merge_params* params, vgicp_merge_stats* stats) {
  note("merge");
  g_dst = dst;
  g_src = src;
  g_params = *params;
  if (stats) {
    *stats = vgicp_merge_stats{};
    stats->voxels = 10; stats->selected = 7; stats->too_far = 2; stats->too_few = 1;
    stats->created = 4; stats->updated = 2; stats->frozen = 1; stats->points = 19;
    stats->seconds = 0.5; stats->device_seconds = 0.25;
  }
  return params->radius == 99.0 ? VGICP_ERR_BAD_ARGUMENT : VGICP_OK;
}
#endif
}

template <typename E, typename F>
static bool throws(F && f, const char * word)
{
  try {
    f();
  } catch (const E & e) {
    return std::strstr(e.what(), word) != nullptr;
  }
  return false;
}

int main() {
  using namespace ESKF_LIO;
  LocalMapConfig onDevice;
  onDevice.deviceResident = true;
  onDevice.keepRawPoints = false;
  LocalMap a(onDevice, false, &g_ctx), b(onDevice, false, &g_other);
  Isometry3d frame = Isometry3d::Identity();
  frame.matrix()(0, 3) = 1.5;
  frame.matrix()(1, 0) = -0.25;
  Vector3d center;
  center(0) = 1.0; center(1) = -2.0; center(2) = 3.0;
  g_calls.clear();
#ifdef WITHOUT_MERGE_LIBRARY
  CHECK(vgicp_map_merge == nullptr);
  CHECK(throws<std::runtime_error>([&] {a.mergeFrom(b, frame, center, 5.0);}, "libvgicp_hip_map_merge.so"));
  CHECK(g_calls.empty());
  std::printf("ok without the library\n");
#else
  const LocalMap::MergeStats st = a.mergeFrom(b, frame, center, 5.0, 2, 40);
  CHECK(g_calls.size() == 1 && g_calls[0] == "merge" && g_dst == &g_ctx && g_src == &g_other);
  CHECK(g_params.center[0] == 1.0 && g_params.center[1] == -2.0 && g_params.center[2] == 3.0 && g_params.radius == 5.0);
  CHECK(g_params.min_count == 2 && g_params.max_count == 40 && g_params.reserved == 0);
  CHECK(g_params.frame[12] == 1.5 && g_params.frame[1] == -0.25 && g_params.frame[0] == 1.0 && g_params.frame[15] == 1.0);   // column-major
  CHECK(st.voxels == 10 && st.selected == 7 && st.tooFar == 2 && st.tooFew == 1 && st.created == 4 && st.updated == 2);
  CHECK(st.frozen == 1 && st.points == 19 && st.seconds == 0.5 && st.deviceSeconds == 0.25);
  // the defaults: every count, no cap; the whole map
  a.mergeFrom(b, frame, center, std::numeric_limits<double>::infinity());
  CHECK(g_params.min_count == 0 && g_params.max_count == 0 && std::isinf(g_params.radius));
  // a refusal of the library comes back as the shim's exception
  CHECK(throws<std::exception>([&] {a.mergeFrom(b, frame, center, 99.0);}, "vgicp_map_merge"));
  // ---- the modes that keep a host shadow grid refuse before the library is asked
  LocalMapConfig shadow;            // deviceResident with keepRawPoints and no rawPointsOnDevice: the default
  CHECK(shadow.deviceResident && shadow.keepRawPoints && !shadow.rawPointsOnDevice);
  LocalMap shadowMap(shadow, false, &g_ctx);
  LocalMapConfig host;
  host.deviceResident = false;
  LocalMap hostMap(host, false, &g_ctx);
  g_calls.clear();
  CHECK(throws<std::runtime_error>([&] {shadowMap.mergeFrom(b, frame, center, 5.0);}, "shadow grid"));
  CHECK(throws<std::runtime_error>([&] {hostMap.mergeFrom(b, frame, center, 5.0);}, "device-resident"));
  CHECK(throws<std::runtime_error>([&] {a.mergeFrom(hostMap, frame, center, 5.0);}, "device-resident"));   // the source on the host
  CHECK(g_calls.empty());
  // a source that keeps a shadow grid is only read: allowed
  a.mergeFrom(shadowMap, frame, center, 5.0);
  CHECK(g_calls.size() == 1);
  std::printf("ok with the library\n");
#endif
  return 0;
}
