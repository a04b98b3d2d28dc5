// The shim's locate members (include/eskf_lio_shim/Registration.hpp: ICP::yawFan / setLocate / locate over
// include/vgicp_hip_map_locate.h) on the CPU, against a stand-in of the C ABI that records the calls: the fan's poses, what
// goes to vgicp_locate_resident, the ranking and its ties, keep, the sequence locate -> levels align x keep -> evaluate,
// the winner, what the members refuse themselves, and that with nothing set no call of the new header is made.
#include <cmath>
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
static int g_locate_rc = VGICP_OK;
static vgicp_locate_params g_params;
static std::vector<double> g_fan;               // the poses vgicp_locate_resident was given
static std::vector<uint32_t> g_hits;            // what it answers per pose
static std::vector<double> g_chain_starts;      // the x translations the chains started from
static std::vector<uint64_t> g_corr;            // what vgicp_evaluate_resident answers per pose ...
static std::vector<double> g_cost;              // ... and its cost
static bool g_planes_asked = false;
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
// pose h scores g_corr[h] correspondences at the cost g_cost[h]
int vgicp_evaluate_resident(vgicp_ctx*, size_t k, const double*, vgicp_evaluation* out, vgicp_eval_stats*) {
  note("evaluate " + std::to_string(k));
  for (size_t h = 0; h < k; ++h) {
    std::memset(&out[h], 0, sizeof out[h]);
    out[h].points = 5;
    out[h].correspondences = h < g_corr.size() ? g_corr[h] : 0;
    out[h].cost = h < g_cost.size() ? g_cost[h] : 0.0;
  }
  return VGICP_OK;
}
int vgicp_map_levels_build(vgicp_ctx*, int levels, vgicp_levels_stats*) { note("levels_build " + std::to_string(levels)); return VGICP_OK; }
// a chain moves its pose by 100 m along z and keeps the rest
int vgicp_align_resident_levels(vgicp_ctx*, const double* guess, size_t stages, const int32_t*, const vgicp_params*, double* pose,
                                vgicp_stats* stats) {
  note("align_resident_levels " + std::to_string(stages));
  g_chain_starts.push_back(guess[12]);
  std::memcpy(pose, guess, 16 * sizeof(double));
  pose[14] += 100.0;
  for (size_t i = 0; i < stages; ++i) {
    stats[i].iterations = 1;
    stats[i].converged = 1;
    stats[i].corr_count[0] = 7;
  }
  return VGICP_OK;
}
// pose h has g_hits[h] hits in the cell of the shift (h, -h, 1), and its pose moved by 10 m per voxel of it
int vgicp_locate_resident(vgicp_ctx*, const double* poses, size_t k, const vgicp_locate_params* params, vgicp_locate_best* best,
                          uint32_t* hits, vgicp_locate_stats* stats) {
  note("locate " + std::to_string(k));
  if (g_locate_rc != VGICP_OK) return g_locate_rc;
  g_params = *params;
  g_fan.assign(poses, poses + 16 * k);
  g_planes_asked = hits != nullptr || stats != nullptr;
  for (size_t h = 0; h < k; ++h) {
    std::memset(&best[h], 0, sizeof best[h]);
    best[h].hits = h < g_hits.size() ? g_hits[h] : 0;
    best[h].offset[0] = (int32_t)h;
    best[h].offset[1] = -(int32_t)h;
    best[h].offset[2] = 1;
    std::memcpy(best[h].pose, poses + 16 * h, 16 * sizeof(double));
    for (int a = 0; a < 3; ++a) best[h].pose[12 + a] += 10.0 * best[h].offset[a];
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
  LocalMapConfig mapConfig;
  LocalMap map(mapConfig, false, &g_ctx);
  PointCloud cloud;
  cloud.points_.assign(5, Vector3d());
  cloud.covariances_.assign(5, Matrix3d());

  // ---- with nothing set: the defaults are kept, and align() makes no call of the new header ----
  RegistrationConfig plain;
  ICP icp(plain);
  CHECK(icp.locateOptions().level == 3 && icp.locateOptions().yaws == 64 && icp.locateOptions().keep == 4 &&
    icp.locateOptions().stride == 1 && icp.locateOptions().window[0] == 4 && icp.locateOptions().window[2] == 1);
  Isometry3d guess = Isometry3d::Identity();
  g_calls.clear();
  (void)icp.align(cloud, map, guess);
  (void)icp.alignCoarseToFine(cloud, map, guess);
  CHECK(count("locate") == 0 && count("align 5") == 2 && g_calls.size() == 2);
  // no schedule anywhere: locate refuses before the library is asked
  CHECK(throws<std::invalid_argument>([&] {(void)icp.locate(cloud, map, guess);}) && g_calls.size() == 2);

  // ---- the fan: pose j is [Rz(2 pi j / count) R | t] ----
  const double a0 = 0.3;
  guess.matrix()(0, 0) = std::cos(a0);
  guess.matrix()(0, 1) = -std::sin(a0);
  guess.matrix()(1, 0) = std::sin(a0);
  guess.matrix()(1, 1) = std::cos(a0);
  guess.matrix()(0, 3) = 1.5;
  guess.matrix()(1, 3) = -2.5;
  guess.matrix()(2, 3) = 0.25;
  const std::vector<Isometry3d> fan = ICP::yawFan(guess, 8);
  CHECK(fan.size() == 8 && std::memcmp(fan[0].matrix().data(), guess.matrix().data(), 16 * sizeof(double)) == 0);
  for (int j = 0; j < 8; ++j) {
    const double a = a0 + 2.0 * 3.14159265358979323846 * j / 8.0;
    const Isometry3d & T = fan[static_cast<size_t>(j)];
    CHECK(std::fabs(T.matrix()(0, 0) - std::cos(a)) < 1e-14 && std::fabs(T.matrix()(1, 0) - std::sin(a)) < 1e-14);
    CHECK(std::fabs(T.matrix()(0, 1) + std::sin(a)) < 1e-14 && std::fabs(T.matrix()(1, 1) - std::cos(a)) < 1e-14);
    CHECK(T.matrix()(2, 2) == 1.0 && T.matrix()(2, 0) == 0.0 && T.matrix()(0, 2) == 0.0 && T.matrix()(3, 3) == 1.0);
    CHECK(T.matrix()(0, 3) == 1.5 && T.matrix()(1, 3) == -2.5 && T.matrix()(2, 3) == 0.25);   // about the sensor's position
  }
  CHECK(throws<std::invalid_argument>([&] {(void)ICP::yawFan(guess, 0);}));

  // ---- locate: one locate, keep chains from the ranked poses, one evaluate ----
  LocateOptions o;
  o.level = 2;
  o.window = {{8, 8, 1}};
  o.stride = 4;
  o.yaws = 8;
  o.keep = 3;
  o.schedule = {2, 1, 0};
  icp.setLocate(o);
  g_hits = {10, 50, 30, 50, 5, 50, 30, 0};      // ranking: 1, 3, 5 (ties to the lower index), then 2, 6, 0, 4, 7
  g_corr = {100, 300, 300};                     // of the chains' ends, in rank order ...
  g_cost = {1.0, 9.0, 4.0};                     // ... candidates 1 and 2 tie on correspondences: the lower cost wins
  g_calls.clear();
  g_chain_starts.clear();
  const Isometry3d pose = icp.locate(cloud, map, guess);
  CHECK(g_calls.size() == 6 && g_calls[0] == "scan_upload 5" && g_calls[1] == "locate 8");
  CHECK(g_calls[2] == "align_resident_levels 3" && g_calls[3] == g_calls[2] && g_calls[4] == g_calls[2] && g_calls[5] == "evaluate 3");
  CHECK(!g_planes_asked);
  CHECK(g_params.level == 2 && g_params.window[0] == 8 && g_params.window[1] == 8 && g_params.window[2] == 1 && g_params.stride == 4);
  CHECK(g_fan.size() == 16 * 8);
  for (size_t j = 0; j < 8; ++j) {CHECK(std::memcmp(&g_fan[16 * j], fan[j].matrix().data(), 16 * sizeof(double)) == 0);}
  // the chains started from the located poses of the fan's poses 1, 3 and 5: x = 1.5 + 10 * index
  CHECK(g_chain_starts == std::vector<double>({11.5, 31.5, 51.5}));
  const std::vector<ICP::LocateCandidate> & found = icp.lastLocation();
  CHECK(found.size() == 3 && found[0].poseIndex == 1 && found[1].poseIndex == 3 && found[2].poseIndex == 5);
  CHECK(found[0].hits == 50 && found[1].offset[0] == 3 && found[1].offset[1] == -3 && found[1].offset[2] == 1);
  CHECK(found[2].start.matrix()(0, 3) == 51.5 && found[2].start.matrix()(2, 3) == 10.25 && found[2].pose.matrix()(2, 3) == 110.25);
  CHECK(found[0].evaluation.correspondences == 100 && found[2].evaluation.cost == 4.0);
  CHECK(icp.lastLocationWinner() == 2 && icp.lastEvaluation().correspondences == 300 && icp.lastEvaluation().cost == 4.0);
  CHECK(pose.matrix()(0, 3) == 51.5 && pose.matrix()(1, 3) == -52.5 && pose.matrix()(2, 3) == 110.25);
  CHECK(pose.matrix()(0, 0) == fan[5].matrix()(0, 0) && icp.lastStages().size() == 3);
  // equal correspondences and equal cost: the better rank stays
  g_cost = {1.0, 4.0, 4.0};
  (void)icp.locate(cloud, map, guess);
  CHECK(icp.lastLocationWinner() == 1);
  // keep above the fan's size: every pose is followed up
  o.yaws = 2;
  o.keep = 8;
  icp.setLocate(o);
  g_calls.clear();
  (void)icp.locate(cloud, map, guess);
  CHECK(count("locate 2") == 1 && count("align_resident_levels") == 2 && count("evaluate 2") == 1);
  // an empty schedule of the options: the ICP's coarse-to-fine schedule
  o.schedule.clear();
  icp.setLocate(o);
  icp.setCoarseToFine({3, 2, 1, 0});
  g_calls.clear();
  (void)icp.locate(cloud, map, guess);
  CHECK(count("align_resident_levels 4") == 2);

  // ---- what the shim refuses itself, and what it makes of the library's refusal ----
  const size_t calls = g_calls.size();
  const LocateOptions kept = icp.locateOptions();
  LocateOptions bad = kept;
  bad.level = 5;
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.window = {{33, 0, 0}};
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.window = {{0, -1, 0}};
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.window = {{10, 10, 5}};
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.stride = 0;
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.yaws = 65;
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.yaws = 0;
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.keep = 9;
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.keep = 0;
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  bad = kept, bad.schedule = {0, 7};
  CHECK(throws<std::invalid_argument>([&] {icp.setLocate(bad);}));
  CHECK(icp.locateOptions().yaws == 2 && icp.locateOptions().keep == 8 && g_calls.size() == calls);   // nothing changed
  RegistrationConfig c;
  c.locate.keep = 9;
  CHECK(throws<std::invalid_argument>([&] {ICP wrong(c);}));
  g_locate_rc = VGICP_ERR_NOT_READY;   // a level the map does not keep
  g_calls.clear();
  CHECK(throws<std::runtime_error>([&] {(void)icp.locate(cloud, map, guess);}));
  CHECK(count("align_resident_levels") == 0 && count("evaluate") == 0);
  g_locate_rc = VGICP_OK;
  std::printf("ok\n");
  return 0;
}
