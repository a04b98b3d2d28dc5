// CPU record of WHICH C-ABI calls the drop-in classes make (include/eskf_lio_shim/LocalMap.hpp, Registration.hpp), in
// which order and with which data, without a device: the whole C ABI the classes touch is replaced by stubs, and every
// stub appends one line to a transcript — its name (without the vgicp_ prefix), its scalar arguments and, for every
// pointer argument, "count:FNV-1a of the bytes".  What the classes print goes into the same transcript.  The program
// plays CloudPreprocessor::process's part itself with shim::stampResident.  Its output is compared byte for byte with
// tests/golden/shim_routes.txt by tests/test_capi_cpu.py, with and without ThreadSanitizer.
//   LocalMap: 8 configurations x 7 clouds x 3 frames (initialize; same pose = no insertion; moved by 1 m = insertion)
//   ICP:      align / alignHypotheses / alignBest / evaluate / alignBestByScore on a stamped, an edited and an unstamped
//             cloud, the size-mismatch messages, and align's "register beside the hash" branch on 3 000 points
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eskf_lio_shim/Registration.hpp"

static std::ostringstream T;   // the transcript (std::cout is pointed at it too)

static uint64_t fnv(const void* p, size_t bytes, uint64_t h = 14695981039346656037ull) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
static std::string hex(uint64_t h) {
  char s[20];
  std::snprintf(s, sizeof s, "%016llx", static_cast<unsigned long long>(h));
  return s;
}
template <typename X>
static std::string H(const X* p, size_t count) {
  if (!p) return "null";
  return std::to_string(count) + ":" + hex(fnv(p, count * sizeof(X)));
}
static void fill(double* p, size_t count, double start) {
  for (size_t i = 0; i < count; ++i) p[i] = start + 0.25 * static_cast<double>(i % 97);
}

// ---- the C ABI, stubbed: every call succeeds, says what it was given, and returns fixed patterns ----
struct vgicp_ctx { int unused; };
static vgicp_ctx g_ctx;
static uint64_t g_generation = 1;     // VGICP_COUNTER_SCAN_GENERATION: the test bumps it ("something replaced the scan")
static size_t g_download = 40;        // points vgicp_scan_download delivers
static size_t g_voxels = 100;         // vgicp_map_size: goes up by 10 with every insertion on the device
static int g_converged = 1;
static std::string P(const vgicp_params* p) {
  return " it=" + std::to_string(p->max_iteration) + " chunk=" + std::to_string(p->chunk_iterations) + " thr=" +
         H(&p->translation_sq_threshold, 2) + " flags=" + std::to_string(p->flags);
}
static void report(vgicp_stats* s) {
  if (!s) return;
  s->iterations = 1;
  s->converged = g_converged;
  s->seconds = 0.5;
  s->device_seconds = 0.25;
  if (s->corr_count) s->corr_count[0] = 42;
}
extern "C" {
int vgicp_create(int, vgicp_ctx** out) { *out = &g_ctx; return VGICP_OK; }
int vgicp_create_multi(const int*, int, vgicp_ctx** out) { *out = &g_ctx; return VGICP_OK; }
int vgicp_destroy(vgicp_ctx*) { return VGICP_OK; }
const char* vgicp_last_error(const vgicp_ctx*) { return ""; }
int vgicp_set_option(vgicp_ctx*, int option, int value) {
  T << "set_option " << option << " " << value << "\n";
  return VGICP_OK;
}
int vgicp_get_counter(const vgicp_ctx*, int which, uint64_t* value) {
  T << "get_counter " << which << "\n";
  if (value) *value = which == VGICP_COUNTER_SCAN_GENERATION ? g_generation : 0;
  return VGICP_OK;
}
int vgicp_map_reset(vgicp_ctx*, double voxel_size, size_t hint) {
  T << "map_reset " << voxel_size << " " << hint << "\n";
  g_voxels = 100;
  return VGICP_OK;
}
int vgicp_map_upsert(vgicp_ctx*, size_t n, const int32_t* keys, const double* means, const double* covs) {
  T << "map_upsert " << n << " k=" << H(keys, 3 * n) << " m=" << H(means, 3 * n) << " c=" << H(covs, 9 * n) << "\n";
  return VGICP_OK;
}
int vgicp_map_erase(vgicp_ctx*, size_t n, const int32_t* keys) {
  T << "map_erase " << n << " k=" << H(keys, 3 * n) << "\n";
  return VGICP_OK;
}
int vgicp_map_size(const vgicp_ctx*, size_t* voxels, size_t* slots) {
  T << "map_size\n";
  if (voxels) *voxels = g_voxels;
  if (slots) *slots = 4096;
  return VGICP_OK;
}
int vgicp_map_export(vgicp_ctx*, size_t capacity, int32_t* keys, double* means, double* covs, uint64_t* counts, size_t* written) {
  const size_t n = capacity < 9 ? capacity : 9;
  T << "map_export " << capacity << "\n";
  std::memset(keys, 0, 3 * n * sizeof(int32_t));
  fill(means, 3 * n, 500.0);
  fill(covs, 9 * n, 1.0);
  for (size_t i = 0; i < n; ++i) counts[i] = 1;
  if (written) *written = n;
  return VGICP_OK;
}
int vgicp_map_points_size(const vgicp_ctx*, size_t* points, size_t* capacity) {
  T << "map_points_size\n";
  if (points) *points = 5;
  if (capacity) *capacity = 64;
  return VGICP_OK;
}
int vgicp_map_points_export(vgicp_ctx*, size_t capacity, int32_t* keys, double* points, size_t* written) {
  T << "map_points_export " << capacity << "\n";
  std::memset(keys, 0, 3 * capacity * sizeof(int32_t));
  fill(points, 3 * capacity, 700.0);
  if (written) *written = capacity;
  return VGICP_OK;
}
int vgicp_map_insert_scan(vgicp_ctx*, size_t n, const double* points, const double* covs, const double* transform, size_t max_points,
                          size_t* new_voxels) {
  T << "map_insert_scan " << n << " p=" << H(points, 3 * n) << " c=" << H(covs, 9 * n) << " T=" << H(transform, 16) << " max=" << max_points
    << " new=" << (new_voxels ? "ptr" : "null") << "\n";
  if (new_voxels) *new_voxels = 0;
  g_voxels += 10;
  return VGICP_OK;
}
int vgicp_map_insert_resident_async(vgicp_ctx*, const double* transform, size_t max_points) {
  T << "map_insert_resident_async T=" << H(transform, 16) << " max=" << max_points << "\n";
  g_voxels += 10;
  return VGICP_OK;
}
int vgicp_map_evict(vgicp_ctx*, const double* position, double distance, size_t* removed) {
  T << "map_evict pos=" << H(position, 3) << " d=" << distance << "\n";
  if (removed) *removed = 7;
  g_voxels -= 7;
  return VGICP_OK;
}
int vgicp_match(vgicp_ctx*, size_t n, const double* points, const double* covs, double*, double*, double*, double*, uint64_t*, size_t* matched) {
  T << "match " << n << " p=" << H(points, 3 * n) << " c=" << H(covs, 9 * n) << "\n";
  if (matched) *matched = 0;
  return VGICP_OK;
}
int vgicp_scan_download(vgicp_ctx*, size_t capacity, double* points, double* covs, size_t* n) {
  T << "scan_download " << capacity << " p=" << (points ? "ptr" : "null") << " c=" << (covs ? "ptr" : "null") << "\n";
  if (points && covs) {
    fill(points, 3 * g_download, -2.0);
    fill(covs, 9 * g_download, 0.5);
  }
  if (n) *n = g_download;
  return VGICP_OK;
}
int vgicp_scan_upload(vgicp_ctx*, size_t n, const double* points, const double* covs) {
  T << "scan_upload " << n << " p=" << H(points, 3 * n) << " c=" << H(covs, 9 * n) << "\n";
  ++g_generation;
  return VGICP_OK;
}
int vgicp_align(vgicp_ctx*, size_t n, const double* points, const double* covs, const double* guess, const vgicp_params* params,
                double* out_pose, vgicp_stats* stats) {
  T << "align " << n << " p=" << H(points, 3 * n) << " c=" << H(covs, 9 * n) << " g=" << H(guess, 16) << P(params) << "\n";
  std::memcpy(out_pose, guess, 16 * sizeof(double));
  report(stats);
  ++g_generation;
  return VGICP_OK;
}
int vgicp_align_resident(vgicp_ctx*, const double* guess, const vgicp_params* params, double* out_pose, vgicp_stats* stats) {
  T << "align_resident g=" << H(guess, 16) << P(params) << "\n";
  std::memcpy(out_pose, guess, 16 * sizeof(double));
  report(stats);
  return VGICP_OK;
}
int vgicp_align_resident_batch(vgicp_ctx*, size_t k, const double* guesses, const vgicp_params* params, double* out_poses,
                               vgicp_batch_stats* stats) {
  T << "align_resident_batch " << k << " g=" << H(guesses, 16 * k) << P(params) << "\n";
  std::memcpy(out_poses, guesses, 16 * k * sizeof(double));
  stats->hypotheses_per_launch = static_cast<int32_t>(k);
  stats->launches = 1;
  stats->seconds = 0.5;
  stats->device_seconds = 0.25;
  for (size_t h = 0; h < k; ++h) {
    stats->status[h] = VGICP_OK;
    stats->iterations[h] = 1;
    stats->converged[h] = g_converged;
    stats->corr_count[h * static_cast<size_t>(params->max_iteration)] = 40 + h;
  }
  return VGICP_OK;
}
int vgicp_evaluate_resident(vgicp_ctx*, size_t k, const double* poses, vgicp_evaluation* out, vgicp_eval_stats* stats) {
  T << "evaluate_resident " << k << " g=" << H(poses, 16 * k) << " stats=" << (stats ? "ptr" : "null") << "\n";
  for (size_t h = 0; h < k; ++h) {
    out[h].points = 50;
    out[h].correspondences = 30 + h;
    out[h].cost = 10.0 - static_cast<double>(h);
    out[h].sq_error = 2.0;
    fill(out[h].normal_eq, 27, static_cast<double>(h));
  }
  return VGICP_OK;
}
}

using namespace ESKF_LIO;

static PointCloudPtr makeCloud(size_t n, int seed) {
  auto cloud = std::make_shared<PointCloud>();
  for (size_t i = 0; i < n; ++i) {
    // a few metres around the origin, several points per 0.5 m voxel
    const double x = -3.0 + 0.37 * static_cast<double>((i * 7 + static_cast<size_t>(seed)) % 17);
    const double y = -2.0 + 0.41 * static_cast<double>((i * 5 + static_cast<size_t>(seed)) % 11);
    const double z = 0.1 * static_cast<double>(i % 3);
    cloud->points_.push_back(Vector3d{{x, y, z}});
    Matrix3d C;
    std::memset(C.m, 0, sizeof C.m);
    C(0, 0) = 1.0 + 0.01 * static_cast<double>(i); C(1, 1) = 1.0; C(2, 2) = 0.5 + 0.001 * seed;
    cloud->covariances_.push_back(C);
  }
  return cloud;
}
static Isometry3d poseAt(double x, double yaw = 0.0) {
  Isometry3d M = Isometry3d::Identity();
  M.matrix()(0, 0) = std::cos(yaw); M.matrix()(0, 1) = -std::sin(yaw);
  M.matrix()(1, 0) = std::sin(yaw); M.matrix()(1, 1) = std::cos(yaw);
  M.matrix()(0, 3) = x;
  return M;
}
static std::string firstPoint(const PointCloud& cloud) {
  if (cloud.points_.empty()) return "none";
  std::ostringstream s;
  s.precision(17);
  s << cloud.points_.size() << "/" << cloud.covariances_.size() << " " << cloud.points_[0](0) << " " << cloud.points_[0](1) << " "
    << cloud.points_[0](2);
  return s.str();
}

enum CloudCase { SoleOwner, SecondOwner, Deferred, Edited, Bumped, Unstamped, Empty, CloudCases };
static const char* kCloudNames[CloudCases] = {"stamped-moved-in", "stamped-caller-keeps", "stamped-deferred", "stamped-edited",
                                              "stamped-generation-bumped", "never-stamped-moved-in", "empty-never-stamped"};

// the part of CloudPreprocessor::process: what the cloud looks like when updateLocalMap gets it
static void prepare(CloudCase which, PointCloud& cloud) {
  switch (which) {
    case SoleOwner:
    case SecondOwner:
      shim::stampResident(&g_ctx, cloud, cloud.points_.size(), true, shim::ResidentCheck::FullHash);
      break;
    case Deferred:   // the host keeps the raw sweep, as process() leaves it with HostCopy::Deferred
      cloud.covariances_.clear();
      shim::stampResident(&g_ctx, cloud, 0, false, shim::ResidentCheck::FullHash);
      break;
    case Edited:
      shim::stampResident(&g_ctx, cloud, cloud.points_.size(), true, shim::ResidentCheck::FullHash);
      reinterpret_cast<unsigned char*>(&cloud.covariances_[17])[3] ^= 0x10;
      break;
    case Bumped:
      shim::stampResident(&g_ctx, cloud, cloud.points_.size(), true, shim::ResidentCheck::FullHash);
      ++g_generation;
      break;
    case Unstamped:
    case Empty:
    case CloudCases:
      shim::forget(&g_ctx);   // (an earlier scenario's stamp must not meet a new cloud at the old one's address)
      break;
  }
}

static void saveAndRecord(const LocalMap& map, const std::string& dir) {
  const std::string pcd = dir + "/routes.pcd", traj = dir + "/routes.json";
  map.save(pcd, traj);
  std::ifstream f(pcd);
  std::vector<std::string> lines;
  std::string line;
  bool data = false;
  while (std::getline(f, line)) {
    if (data) lines.push_back(line);
    if (line.rfind("DATA", 0) == 0) data = true;
  }
  std::sort(lines.begin(), lines.end());
  uint64_t h = 14695981039346656037ull;
  for (const auto& l : lines) h = fnv("\n", 1, fnv(l.data(), l.size(), h));
  T << "saved " << lines.size() << " points " << hex(h) << "\n";
}

static void mapScenarios(const std::string& dir) {
  struct MapCase { const char* name; bool deviceResident, keepRawPoints, rawOnDevice; };
  const MapCase maps[4] = {{"defaults", true, true, false}, {"rawPointsOnDevice", true, true, true},
                           {"deviceResident-no-raw-points", true, false, false}, {"host-authoritative", false, true, false}};
  for (const MapCase& m : maps) {
    for (int eviction = 0; eviction < 2; ++eviction) {
      for (int c = 0; c < CloudCases; ++c) {
        LocalMapConfig config;
        config.voxelSize = 0.5;
        config.maxNumPointsPerVoxel = 3;
        config.distanceThreshold = 3.0;
        config.deviceResident = m.deviceResident;
        config.keepRawPoints = m.keepRawPoints;
        config.rawPointsOnDevice = m.rawOnDevice;
        if (eviction) {config.removePeriod = 0.0;} else {config.removeDistantPoints = false;}
        T << "== map " << m.name << (eviction ? " removePeriod=0" : " removeDistantPoints=false") << " cloud " << kCloudNames[c] << "\n";
        LocalMap map(config, false, &g_ctx);
        const Isometry3d poses[3] = {poseAt(0.0, 0.1), poseAt(0.0, 0.1), poseAt(1.0, 0.1)};
        for (int frame = 0; frame < 3; ++frame) {
          T << "-- frame " << frame + 1 << "\n";
          PointCloudPtr cloud = makeCloud(c == Empty ? 0 : 50, frame);
          prepare(static_cast<CloudCase>(c), *cloud);
          PointCloudPtr kept;
          const bool movedIn = c == SoleOwner || c == Unstamped;
          if (!movedIn) kept = cloud;
          map.updateLocalMap(std::move(cloud), poses[frame], frame == 0);
          const size_t size = map.size();
          T << "savesRawPoints " << map.savesRawPoints() << " size " << size << " cloud " << (kept ? firstPoint(*kept) : std::string("moved in")) << "\n";
        }
        saveAndRecord(map, dir);
      }
    }
  }
}

template <typename Call>
static void guarded(const char* what, Call call) {
  T << "-- " << what << "\n";
  try {
    call();
  } catch (const std::exception& e) {
    T << "threw " << e.what() << "\n";
  }
}
static void recordStats(const ICP& icp) {
  const ICP::Stats& s = icp.lastStats();
  T << "resident " << icp.lastUsedResidentScan() << " iterations " << s.iterations << " converged " << s.converged << " counts "
    << H(s.correspondenceCounts.data(), s.correspondenceCounts.size()) << " best " << icp.lastBestHypothesis() << " per-launch "
    << icp.lastHypothesesPerLaunch() << "\n";
}

// every method meets a cloud as `fresh` makes it: a method that uploads replaces the resident scan
template <typename Fresh>
static void icpMethods(ICP& icp, const LocalMap& map, Fresh fresh) {
  const std::vector<Isometry3d> guesses = {poseAt(0.0), poseAt(0.5, 0.2), poseAt(1.0, -0.2)};
  const std::vector<Isometry3d> two = {poseAt(0.25), poseAt(0.75, 0.3)};
  PointCloudPtr cloud = fresh();
  guarded("align", [&] {
    const Isometry3d out = icp.align(*cloud, map, guesses[1]);
    T << "pose " << H(shim::poseData(out), 16) << "\n";
    recordStats(icp);
  });
  cloud = fresh();
  guarded("alignHypotheses", [&] {
    const auto all = icp.alignHypotheses(*cloud, map, guesses);
    for (const auto& h : all) {
      T << "hypothesis " << H(shim::poseData(h.pose), 16) << " " << h.converged << " " << h.iterations << " " << h.finalCorrespondences << "\n";
    }
    recordStats(icp);
  });
  cloud = fresh();
  guarded("alignBest", [&] {
    const Isometry3d out = icp.alignBest(*cloud, map, guesses);
    T << "pose " << H(shim::poseData(out), 16) << "\n";
    recordStats(icp);
  });
  cloud = fresh();
  guarded("evaluate", [&] {
    const auto scores = icp.evaluate(*cloud, map, two);
    for (const auto& e : scores) {
      T << "evaluation " << e.points << " " << e.correspondences << " " << e.cost << " " << e.squaredError << " "
        << H(e.normalEquations.data(), e.normalEquations.size()) << "\n";
    }
    recordStats(icp);
  });
  cloud = fresh();
  guarded("alignBestByScore", [&] {
    const Isometry3d out = icp.alignBestByScore(*cloud, map, guesses);
    T << "pose " << H(shim::poseData(out), 16) << " score " << icp.lastEvaluation().score() << "\n";
    recordStats(icp);
  });
}

static void icpScenarios() {
  LocalMapConfig config;
  T << "== ICP\n";
  LocalMap map(config, false, &g_ctx);
  RegistrationConfig rc;
  rc.maxIteration = 5;
  rc.chunkIterations = 2;
  const CloudCase cases[3] = {SecondOwner, Edited, Unstamped};
  for (CloudCase c : cases) {
    T << "== ICP cloud " << kCloudNames[c] << "\n";
    ICP icp(rc);
    icpMethods(icp, map, [&] {
      PointCloudPtr cloud = makeCloud(50, 3);
      prepare(c, *cloud);
      return cloud;
    });
  }
  {
    T << "== ICP cloud with 50 points and 49 covariances\n";
    ICP icp(rc);
    icpMethods(icp, map, [&] {
      PointCloudPtr cloud = makeCloud(50, 4);
      cloud->covariances_.pop_back();
      prepare(Unstamped, *cloud);
      return cloud;
    });
  }
  {
    T << "== ICP not converged\n";
    ICP icp(rc);
    g_converged = 0;
    icpMethods(icp, map, [&] {
      PointCloudPtr cloud = makeCloud(50, 5);
      prepare(Unstamped, *cloud);
      return cloud;
    });
    g_converged = 1;
  }
  // align's "register beside the hash" branch: at least 256 KiB of cloud and helper threads
  for (int helpers : {2, 0}) {
    for (int edited = 0; edited < 2; ++edited) {
      T << "== ICP 3000 points, helpers " << helpers << (edited ? ", edited in place" : "") << "\n";
      shim::HashCrew::instance().setHelpers(helpers);
      ICP icp(rc);
      PointCloudPtr cloud = makeCloud(3000, 6);
      shim::stampResident(&g_ctx, *cloud, 3000, true, shim::ResidentCheck::FullHash);
      if (edited) reinterpret_cast<unsigned char*>(&cloud->covariances_[2017])[5] ^= 0x01;
      guarded("align", [&] {
        const Isometry3d out = icp.align(*cloud, map, poseAt(0.5, 0.2));
        T << "pose " << H(shim::poseData(out), 16) << "\n";
        recordStats(icp);
      });
    }
  }
  shim::HashCrew::instance().setHelpers(2);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  std::streambuf* out = std::cout.rdbuf(T.rdbuf());   // "removed N voxels", "ICP not converged!"
  mapScenarios(dir);
  icpScenarios();
  std::cout.rdbuf(out);
  const std::string text = T.str();
  std::fwrite(text.data(), 1, text.size(), stdout);
  return 0;
}
