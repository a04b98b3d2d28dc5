// The shim's coarse-to-fine members (include/eskf_lio_shim/LocalMap.hpp: LocalMap::setLevels;
// include/eskf_lio_shim/Registration.hpp: ICP::setCoarseToFine / alignCoarseToFine over include/vgicp_hip_map_levels.h) on
// the CPU, against a stand-in of the C ABI that records the calls: what the members hand to vgicp_map_levels_build and
// vgicp_align_resident_levels, what they make of the answer, what they refuse themselves, and that with nothing set no
// call of the new header is made.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "eskf_lio_shim/Registration.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// ---- the C ABI, stubbed: every call leaves one line ----
struct vgicp_ctx { int unused; };
static vgicp_ctx g_ctx;
static std::vector<std::string> g_calls;
static int g_build_rc = VGICP_OK, g_levels_rc = VGICP_OK;
static std::vector<int32_t> g_last_levels;
static std::vector<vgicp_params> g_last_params;
static double g_last_guess[16];
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
int vgicp_map_insert_scan(vgicp_ctx*, size_t, const double*, const double*, const double*, size_t, size_t* new_voxels) { if (new_voxels) *new_voxels = 0; return VGICP_OK; }
int vgicp_map_insert_resident_async(vgicp_ctx*, const double*, size_t) { return VGICP_OK; }
int vgicp_map_evict(vgicp_ctx*, const double*, double, size_t* removed) { if (removed) *removed = 0; return VGICP_OK; }
int vgicp_match(vgicp_ctx*, size_t, const double*, const double*, double*, double*, double*, double*, uint64_t*, size_t* matched) { if (matched) *matched = 0; return VGICP_OK; }
int vgicp_get_counter(const vgicp_ctx*, int, uint64_t* value) { if (value) *value = 0; return VGICP_OK; }
int vgicp_scan_download(vgicp_ctx*, size_t, double*, double*, size_t* n) { if (n) *n = 0; return VGICP_ERR_NOT_READY; }
int vgicp_scan_upload(vgicp_ctx*, size_t n, const double*, const double*) { note("scan_upload " + std::to_string(n)); return VGICP_OK; }
int vgicp_align(vgicp_ctx*, size_t n, const double*, const double*, const double* guess, const vgicp_params*, double* pose, vgicp_stats* stats) {
  note("align " + std::to_string(n));
  std::memcpy(pose, guess, 16 * sizeof(double));
  stats->iterations = 1;
  stats->converged = 1;
  return VGICP_OK;
}
int vgicp_align_resident(vgicp_ctx*, const double* guess, const vgicp_params*, double* pose, vgicp_stats* stats) {
  note("align_resident");
  std::memcpy(pose, guess, 16 * sizeof(double));
  stats->iterations = 1;
  stats->converged = 1;
  return VGICP_OK;
}
int vgicp_align_resident_batch(vgicp_ctx*, size_t, const double*, const vgicp_params*, double*, vgicp_batch_stats*) { return VGICP_OK; }
int vgicp_align_batch_width(vgicp_ctx*, size_t* w) { if (w) *w = 1; return VGICP_OK; }
int vgicp_evaluate_resident(vgicp_ctx*, size_t, const double*, vgicp_evaluation*, vgicp_eval_stats*) { return VGICP_OK; }
int vgicp_map_levels_build(vgicp_ctx*, int levels, vgicp_levels_stats* stats) {
  note("levels_build " + std::to_string(levels) + (stats ? " stats" : ""));
  return g_build_rc;
}
int vgicp_align_resident_levels(vgicp_ctx*, const double* guess, size_t stages, const int32_t* levels, const vgicp_params* params,
                                double* pose, vgicp_stats* stats) {
  note("align_resident_levels " + std::to_string(stages));
  if (g_levels_rc != VGICP_OK) return g_levels_rc;
  std::memcpy(g_last_guess, guess, sizeof g_last_guess);
  g_last_levels.assign(levels, levels + stages);
  g_last_params.assign(params, params + stages);
  std::memcpy(pose, guess, 16 * sizeof(double));
  pose[12] += 1.0;   // the chain moved the pose by one metre along x
  for (size_t i = 0; i < stages; ++i) {
    stats[i].iterations = (int32_t)(i + 2);
    stats[i].converged = i + 1 == stages ? 0 : 1;
    stats[i].seconds = 0.5 * (double)(i + 1);
    stats[i].device_seconds = 0.25 * (double)(i + 1);
    for (size_t r = 0; r < i + 2; ++r) stats[i].corr_count[r] = 100 * (i + 1) + r;
  }
  return VGICP_OK;
}
}

template <typename E, typename F>
static bool throws(F && f)
{
  try {
    f();
  } catch (const E &) {
    return true;
  }
  return false;
}
static size_t count(const char * prefix)
{
  size_t n = 0;
  for (const std::string & s : g_calls) {n += s.rfind(prefix, 0) == 0;}
  return n;
}

int main() {
  using namespace ESKF_LIO;
  // ---- with nothing set: no call of the new header, and alignCoarseToFine without a schedule is align() ----
  LocalMapConfig plainMap;
  LocalMap map(plainMap, false, &g_ctx);
  CHECK(map.levels() == 0 && count("levels_build") == 0 && g_calls.size() == 1 && g_calls[0] == "map_reset");
  RegistrationConfig plain;
  ICP icp(plain);
  CHECK(icp.coarseToFineLevels().empty());
  PointCloud cloud;
  cloud.points_.assign(5, Vector3d());
  cloud.covariances_.assign(5, Matrix3d());
  Isometry3d guess = Isometry3d::Identity();
  guess.matrix()(1, 3) = 0.75;
  g_calls.clear();
  (void)icp.alignCoarseToFine(cloud, map, guess);
  CHECK(count("align_resident_levels") == 0 && count("align 5") == 1);

  // ---- LocalMap::setLevels ----
  g_calls.clear();
  map.setLevels(3);
  CHECK(map.levels() == 3 && g_calls.size() == 1 && g_calls[0] == "levels_build 3");
  CHECK(throws<std::invalid_argument>([&] {map.setLevels(-1);}) && throws<std::invalid_argument>([&] {map.setLevels(VGICP_LEVELS_MAX + 1);}));
  CHECK(map.levels() == 3 && g_calls.size() == 1);          // refused before the library is asked; nothing changed
  g_build_rc = VGICP_ERR_BAD_ARGUMENT;                      // the library's own refusal (a multi-device context) is an error
  CHECK(throws<std::runtime_error>([&] {map.setLevels(2);}) && map.levels() == 3);
  g_build_rc = VGICP_OK;
  map.setLevels(0);
  CHECK(map.levels() == 0 && g_calls.back() == "levels_build 0");
  LocalMapConfig withLevels;
  withLevels.levels = 2;
  g_calls.clear();
  LocalMap second(withLevels, false, &g_ctx);
  CHECK(second.levels() == 2 && g_calls.size() == 2 && g_calls[0] == "map_reset" && g_calls[1] == "levels_build 2");

  // ---- ICP::alignCoarseToFine with a schedule ----
  map.setLevels(3);
  RegistrationConfig c;
  c.maxIteration = 77;
  c.translationSquaredThreshold = 3.0e-6;
  c.cosineThreshold = 0.99995;
  c.coarseToFineLevels = {3, 2, 1, 0};
  c.coarseMaxIteration = 12;
  c.coarseTranslationSquaredThreshold = 2.0e-4;
  c.coarseCosineThreshold = 0.998;
  ICP ctf(c);
  CHECK(ctf.coarseToFineLevels().size() == 4);
  g_calls.clear();
  const Isometry3d pose = ctf.alignCoarseToFine(cloud, map, guess);
  // the cloud was never prepared on the device: ONE upload, then the one call
  CHECK(g_calls.size() == 2 && g_calls[0] == "scan_upload 5" && g_calls[1] == "align_resident_levels 4");
  CHECK(!ctf.lastUsedResidentScan());
  CHECK(std::memcmp(g_last_guess, guess.matrix().data(), sizeof g_last_guess) == 0);
  CHECK(g_last_levels == std::vector<int32_t>({3, 2, 1, 0}));
  for (int i = 0; i < 3; ++i) {
    CHECK(g_last_params[i].max_iteration == 12 && g_last_params[i].translation_sq_threshold == 2.0e-4 &&
      g_last_params[i].cosine_threshold == 0.998 && g_last_params[i].flags == 0);
  }
  CHECK(g_last_params[3].max_iteration == 77 && g_last_params[3].translation_sq_threshold == 3.0e-6 &&
    g_last_params[3].cosine_threshold == 0.99995);
  CHECK(pose.matrix()(0, 3) == 1.0 && pose.matrix()(1, 3) == 0.75);
  CHECK(ctf.lastStages().size() == 4 && ctf.lastStages()[0].level == 3 && ctf.lastStages()[3].level == 0);
  CHECK(ctf.lastStages()[1].stats.iterations == 3 && ctf.lastStages()[1].stats.converged);
  CHECK(ctf.lastStages()[1].stats.correspondenceCounts == std::vector<uint64_t>({200, 201, 202}));
  CHECK(ctf.lastStats().iterations == 5 && !ctf.lastStats().converged && ctf.lastStats().seconds == 2.0 &&
    ctf.lastStats().deviceSeconds == 1.0 && ctf.lastStats().correspondenceCounts.size() == 5);
  // a schedule of the call's own: free order, a single stage takes the fine thresholds
  (void)ctf.alignCoarseToFine(cloud, map, guess, {1, 3, 1});
  CHECK(g_last_levels == std::vector<int32_t>({1, 3, 1}) && g_last_params[2].max_iteration == 77 && g_last_params[1].max_iteration == 12);
  (void)ctf.alignCoarseToFine(cloud, map, guess, {2});
  CHECK(g_last_levels == std::vector<int32_t>({2}) && g_last_params[0].max_iteration == 77);

  // ---- what the shim refuses itself, and what it makes of the library's refusal ----
  const size_t calls = g_calls.size();
  CHECK(throws<std::invalid_argument>([&] {(void)ctf.alignCoarseToFine(cloud, map, guess, {});}));
  CHECK(throws<std::invalid_argument>([&] {(void)ctf.alignCoarseToFine(cloud, map, guess, {0, 5});}));
  CHECK(throws<std::invalid_argument>([&] {(void)ctf.alignCoarseToFine(cloud, map, guess, {0, -1});}));
  CHECK(throws<std::invalid_argument>([&] {(void)ctf.alignCoarseToFine(cloud, map, guess, std::vector<int>(9, 0));}));
  CHECK(throws<std::invalid_argument>([&] {ctf.setCoarseToFine({0, 7});}) && ctf.coarseToFineLevels().size() == 4);
  CHECK(throws<std::invalid_argument>([&] {ctf.setCoarseToFine({1, 0}, -1);}) && ctf.coarseToFineLevels().size() == 4);
  CHECK(g_calls.size() == calls);
  c.coarseToFineLevels = {9};
  CHECK(throws<std::invalid_argument>([&] {ICP bad(c);}));
  g_levels_rc = VGICP_ERR_NOT_READY;   // a level the map does not keep
  CHECK(throws<std::runtime_error>([&] {(void)ctf.alignCoarseToFine(cloud, map, guess);}));
  g_levels_rc = VGICP_OK;
  ctf.setCoarseToFine({});
  g_calls.clear();
  (void)ctf.alignCoarseToFine(cloud, map, guess);
  CHECK(count("align_resident_levels") == 0 && count("align 5") == 1);
  std::printf("ok\n");
  return 0;
}
