// vgicp_host.cpp — builds the C++ host mirror (include/eskf_lio_shim/: ESKF_LIO::LocalMap,
// ESKF_LIO::ICP and ESKF_LIO::CloudPreprocessor with the reference's method signatures) into libvgicp_host.so and gives it a small
// C surface so the Python parity tests can drive the SAME C++ objects a patched Odometry.cpp would
// (reference call sites: src/Odometry.cpp:61,86, src/ErrorStateKF.cpp:130).
// Compiled with plain g++ against the dependency-free stand-in types (no Eigen / Open3D here); all
// compute goes through libvgicp_hip.so.
#define ESKF_LIO_SHIM_FORCE_POD 1
#include <cstring>
#include <deque>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../include/eskf_lio_shim/CloudPreprocessor.hpp"
#include "../../include/eskf_lio_shim/Registration.hpp"
#include "../csrc/vgicp_math.h"

using ESKF_LIO::CloudPreprocessor;
using ESKF_LIO::ICP;
using ESKF_LIO::Isometry3d;
using ESKF_LIO::LocalMap;
using ESKF_LIO::PointCloud;

namespace
{
thread_local std::string g_error;

PointCloud makeCloud(size_t n, const double * points, const double * covs)
{
  PointCloud cloud;
  cloud.points_.resize(n);
  cloud.covariances_.resize(n);
  if (n) {
    std::memcpy(cloud.points_.data(), points, n * 24);
    std::memcpy(cloud.covariances_.data(), covs, n * 72);
  }
  return cloud;
}

template<typename F>
int guarded(F && f)
{
  try {
    f();
    return 0;
  } catch (const std::exception & e) {
    g_error = e.what();
    return 1;
  }
}
}  // namespace

extern "C" {

const char * host_last_error(void) {return g_error.c_str();}

// LocalMap(config) — the YAML constructor's keys as plain arguments, with LocalMapConfig::rawPointsOnDevice (the device
// map keeps the raw points save() writes).
LocalMap * host_localmap_create_config_raw(
  double voxel_size, size_t max_points_per_voxel, double translation_sq_threshold,
  double cosine_threshold, int remove_distant_points, double distance_threshold,
  double remove_period, int device_resident, int keep_raw_points, int raw_points_on_device)
{
  LocalMap * out = nullptr;
  guarded(
    [&] {
      ESKF_LIO::LocalMapConfig c;
      c.voxelSize = voxel_size;
      c.maxNumPointsPerVoxel = max_points_per_voxel;
      c.translationSquaredThreshold = translation_sq_threshold;
      c.cosineThreshold = cosine_threshold;
      c.removeDistantPoints = remove_distant_points != 0;
      c.distanceThreshold = distance_threshold;
      c.removePeriod = remove_period;
      c.deviceResident = device_resident != 0;
      c.keepRawPoints = keep_raw_points != 0;
      c.rawPointsOnDevice = raw_points_on_device != 0;
      out = new LocalMap(c);
    });
  return out;
}

// The same without rawPointsOnDevice (the signature of the earlier library).
LocalMap * host_localmap_create_config(
  double voxel_size, size_t max_points_per_voxel, double translation_sq_threshold,
  double cosine_threshold, int remove_distant_points, double distance_threshold,
  double remove_period, int device_resident, int keep_raw_points)
{
  return host_localmap_create_config_raw(
    voxel_size, max_points_per_voxel, translation_sq_threshold, cosine_threshold, remove_distant_points,
    distance_threshold, remove_period, device_resident, keep_raw_points, 0);
}

// LocalMap(double voxelSize, size_t maxNumPointsPerVoxel, bool visualize = false)
LocalMap * host_localmap_create(double voxel_size, size_t max_points_per_voxel)
{
  LocalMap * out = nullptr;
  guarded([&] {out = new LocalMap(voxel_size, max_points_per_voxel);});
  return out;
}

void host_localmap_destroy(LocalMap * map) {delete map;}
// helper threads of the drop-in's full-hash check (CloudPreprocessorConfig::residentCheckThreads; 0 = the caller alone)
void host_hash_helpers(int n) {ESKF_LIO::shim::HashCrew::instance().setHelpers(n);}
size_t host_localmap_size(const LocalMap * map) {return map->size();}
int host_localmap_saves_raw_points(const LocalMap * map) {return map->savesRawPoints() ? 1 : 0;}
// waits until the shadow grid's worker has filed every cloud handed to it (what LocalMap::grid() / save() do first);
// returns the host grid's voxel count
size_t host_localmap_drain(const LocalMap * map) {return map->grid().size();}
// LocalMap::setInsertGate / insertGate / gatedTotals (include/vgicp_hip_map_gated.h); out: points, refused, plain frames
int host_localmap_set_insert_gate(LocalMap * map, double gate) {return guarded([&] {map->setInsertGate(gate);});}
double host_localmap_insert_gate(const LocalMap * map) {return map->insertGate();}
int host_localmap_gated_totals(const LocalMap * map, uint64_t out[3])
{
  return guarded(
    [&] {
      const LocalMap::GatedTotals t = map->gatedTotals();
      out[0] = t.points;
      out[1] = t.refused;
      out[2] = t.plainFrames;
    });
}

// LocalMap::setCarve / clearCarve / carveTotals (include/vgicp_hip_map_carve.h); out: rays, removed
int host_localmap_set_carve(
  LocalMap * map, double margin, double max_range, uint32_t min_hits, uint32_t stride, const double origin[3])
{
  return guarded(
    [&] {
      const vgicp_carve_params p = {{origin[0], origin[1], origin[2]}, margin, max_range, min_hits, stride};
      map->setCarve(p);
    });
}
void host_localmap_clear_carve(LocalMap * map) {map->clearCarve();}
int host_localmap_carve_totals(const LocalMap * map, uint64_t out[2])
{
  return guarded(
    [&] {
      const LocalMap::CarveTotals t = map->carveTotals();
      out[0] = t.rays;
      out[1] = t.removed;
    });
}

// LocalMap::rayReport / rayCounts (include/vgicp_hip_map_rays.h).  params: origin (3), margin, beyond, max_range.
// *available = 0: the map or the scan is not on the device, nothing is written.  ray_report: capacity points of room in
// every plane (NULL: not wanted), *n the report's points; counts: rays, visits, by_class[8] per transform.
int host_localmap_ray_report(
  const LocalMap * map, const double transform[16], const double params[6], uint32_t stride, size_t capacity,
  uint8_t * status, double * range, int32_t * hit_key, uint32_t * steps, uint64_t counts[10], size_t * n, int * available)
{
  return guarded(
    [&] {
      const vgicp_ray_params p = {{params[0], params[1], params[2]}, params[3], params[4], params[5], stride, 0};
      const LocalMap::RayReport r = map->rayReport(ESKF_LIO::shim::poseFromData(transform), p);
      *available = r.available ? 1 : 0;
      *n = r.status.size();
      if (!r.available) {return;}
      const size_t m = std::min(capacity, r.status.size());
      if (status && m) {std::memcpy(status, r.status.data(), m);}
      if (range && m) {std::memcpy(range, r.range.data(), m * sizeof(double));}
      if (hit_key && m) {std::memcpy(hit_key, r.hitKey.data(), m * 3 * sizeof(int32_t));}
      if (steps && m) {std::memcpy(steps, r.steps.data(), m * sizeof(uint32_t));}
      counts[0] = r.counts.rays;
      counts[1] = r.counts.visits;
      for (int k = 0; k < 8; ++k) {counts[2 + k] = r.counts.byClass[k];}
    });
}
int host_localmap_ray_counts(
  const LocalMap * map, size_t k, const double * transforms, const double params[6], uint32_t stride, uint64_t * counts,
  int * available)
{
  return guarded(
    [&] {
      const vgicp_ray_params p = {{params[0], params[1], params[2]}, params[3], params[4], params[5], stride, 0};
      std::vector<Isometry3d> T(k);
      for (size_t h = 0; h < k; ++h) {T[h] = ESKF_LIO::shim::poseFromData(transforms + 16 * h);}
      const LocalMap::RayCountsList r = map->rayCounts(T, p);
      *available = r.available ? 1 : 0;
      for (size_t h = 0; h < r.counts.size(); ++h) {
        counts[10 * h] = r.counts[h].rays;
        counts[10 * h + 1] = r.counts[h].visits;
        for (int c = 0; c < 8; ++c) {counts[10 * h + 2 + c] = r.counts[h].byClass[c];}
      }
    });
}

// updateLocalMap(cloud, transform, initialize); the transformed cloud is written back to
// points/covs, as the reference mutates the shared cloud in place (src/LocalMap.cpp:15).
int host_localmap_update(
  LocalMap * map, size_t n, double * points, double * covs, const double transform[16],
  int initialize)
{
  return guarded(
    [&] {
      auto cloud = std::make_shared<PointCloud>(makeCloud(n, points, covs));
      map->updateLocalMap(cloud, ESKF_LIO::shim::poseFromData(transform), initialize != 0);
      if (n) {
        std::memcpy(points, cloud->points_.data(), n * 24);
        std::memcpy(covs, cloud->covariances_.data(), n * 72);
      }
    });
}

// correspondenceMatching(points, covariances) -> the four arrays, M returned through *matched.
int host_localmap_match(
  const LocalMap * map, size_t n, const double * points, const double * covs, double * src_points,
  double * src_covs, double * map_points, double * map_covs, size_t * matched)
{
  return guarded(
    [&] {
      PointCloud cloud = makeCloud(n, points, covs);
      auto [sp, sc, mp, mc] = map->correspondenceMatching(cloud.points_, cloud.covariances_);
      *matched = sp.size();
      if (!sp.empty()) {
        std::memcpy(src_points, sp.data(), sp.size() * 24);
        std::memcpy(src_covs, sc.data(), sc.size() * 72);
        std::memcpy(map_points, mp.data(), mp.size() * 24);
        std::memcpy(map_covs, mc.data(), mc.size() * 72);
      }
    });
}

// Host-authoritative voxel statistics (order = container iteration order).
size_t host_localmap_export(
  const LocalMap * map, size_t capacity, int32_t * keys, double * means, double * covs,
  uint64_t * counts)
{
  size_t w = 0;
  if (map->deviceResident()) {
    if (vgicp_map_export(map->context(), capacity, keys, means, covs, counts, &w) != VGICP_OK) {return 0;}
    return w;
  }
  for (const auto & kv : map->grid()) {
    if (w == capacity) {break;}
    keys[3 * w] = kv.first.i;
    keys[3 * w + 1] = kv.first.j;
    keys[3 * w + 2] = kv.first.k;
    std::memcpy(means + 3 * w, kv.second.mean.data(), 24);
    std::memcpy(covs + 9 * w, kv.second.covariance.data(), 72);
    counts[w] = kv.second.numPoints;
    ++w;
  }
  return w;
}

int host_localmap_save(const LocalMap * map, const char * cloud_path, const char * trajectory_path)
{
  return guarded([&] {map->save(cloud_path, trajectory_path);});
}

// vgicp_get_counter of the map's device context (0 where the map has none)
uint64_t host_localmap_counter(const LocalMap * map, int which)
{
  uint64_t v = 0;
  guarded([&] {if (map->context()) {vgicp_get_counter(map->context(), which, &v);}});
  return v;
}

// ICP(config) — registration.max_iteration / translation_sq_threshold / cosine_threshold
ICP * host_icp_create(
  int max_iteration, double translation_sq_threshold, double cosine_threshold, int chunk_iterations)
{
  ESKF_LIO::RegistrationConfig c;
  c.maxIteration = max_iteration;
  c.translationSquaredThreshold = translation_sq_threshold;
  c.cosineThreshold = cosine_threshold;
  c.chunkIterations = chunk_iterations;
  return new ICP(c);
}
// The same with the optional keys registration.robust_kernel (NULL = absent) / robust_scale / gate, as the YAML
// constructor reads them.
ICP * host_icp_create_robust(
  int max_iteration, double translation_sq_threshold, double cosine_threshold, int chunk_iterations,
  const char * robust_kernel, double robust_scale, double gate)
{
  ICP * out = nullptr;
  guarded(
    [&] {
      ESKF_LIO::RegistrationConfig c;
      c.maxIteration = max_iteration;
      c.translationSquaredThreshold = translation_sq_threshold;
      c.cosineThreshold = cosine_threshold;
      c.chunkIterations = chunk_iterations;
      if (robust_kernel) {c.robustKernel = ESKF_LIO::RegistrationConfig::robustKernelFromName(robust_kernel);}
      c.robustScale = robust_scale;
      c.robustGate = gate;
      out = new ICP(c);
    });
  return out;
}
// icp->setRobust(kind, scale, gate); out3 (optional): kind, scale and gate as the library will use them
int host_icp_set_robust(ICP * icp, int kind, double scale, double gate, double * out3)
{
  return guarded(
    [&] {
      icp->setRobust(kind, scale, gate);
      if (out3) {
        out3[0] = icp->robustKernel();
        out3[1] = icp->robustScale();
        out3[2] = icp->robustGate();
      }
    });
}
int host_icp_hypotheses_per_launch(const ICP * icp) {return icp->lastHypothesesPerLaunch();}
void host_icp_destroy(ICP * icp) {delete icp;}

// icp->align(cloud, localMap, guess)
int host_icp_align(
  ICP * icp, size_t n, const double * points, const double * covs, const LocalMap * map,
  const double guess[16], double out_pose[16], int32_t * iterations, int32_t * converged,
  uint64_t * corr_count, size_t corr_capacity)
{
  return guarded(
    [&] {
      const PointCloud cloud = makeCloud(n, points, covs);
      const Isometry3d T = icp->align(cloud, *map, ESKF_LIO::shim::poseFromData(guess));
      std::memcpy(out_pose, ESKF_LIO::shim::poseData(T), 16 * sizeof(double));
      const auto & st = icp->lastStats();
      if (iterations) {*iterations = st.iterations;}
      if (converged) {*converged = st.converged ? 1 : 0;}
      for (size_t k = 0; k < st.correspondenceCounts.size() && k < corr_capacity; ++k) {
        corr_count[k] = st.correspondenceCounts[k];
      }
    });
}

// icp->alignWithPrior(cloud, localMap, guess, information) (information: column-major 6 x 6), then
// icp->posteriorInformation() into out_posterior (column-major 6 x 6); *has_prior: icp->hasPrior() afterwards.
int host_icp_align_with_prior(
  ICP * icp, size_t n, const double * points, const double * covs, const LocalMap * map,
  const double guess[16], const double information[36], double out_pose[16], double out_posterior[36],
  int32_t * iterations, int32_t * converged, int32_t * has_prior)
{
  return guarded(
    [&] {
      const PointCloud cloud = makeCloud(n, points, covs);
      ESKF_LIO::Matrix6d info = ESKF_LIO::Matrix6d::Zero();
      for (int k = 0; k < 36; ++k) {info.data()[k] = information[k];}
      const Isometry3d T = icp->alignWithPrior(cloud, *map, ESKF_LIO::shim::poseFromData(guess), info);
      std::memcpy(out_pose, ESKF_LIO::shim::poseData(T), 16 * sizeof(double));
      const ESKF_LIO::Matrix6d post = icp->posteriorInformation();
      for (int k = 0; k < 36; ++k) {out_posterior[k] = post.data()[k];}
      if (iterations) {*iterations = icp->lastStats().iterations;}
      if (converged) {*converged = icp->lastStats().converged ? 1 : 0;}
      if (has_prior) {*has_prior = icp->hasPrior() ? 1 : 0;}
    });
}

// icp->alignHypotheses(cloud, localMap, guesses) / icp->alignBest(...) on a cloud built from the arrays (not resident:
// one upload).  out_poses k x 16, iterations / converged / final_corr k entries (each optional); with best != NULL the
// call is alignBest: *best receives the chosen index and best_pose its pose.
int host_icp_align_hypotheses(
  ICP * icp, size_t n, const double * points, const double * covs, const LocalMap * map, size_t k,
  const double * guesses, double * out_poses, int32_t * iterations, int32_t * converged, uint64_t * final_corr,
  int32_t * best, double best_pose[16], int32_t * used_resident)
{
  return guarded(
    [&] {
      const PointCloud cloud = makeCloud(n, points, covs);
      std::vector<Isometry3d> g(k);
      for (size_t h = 0; h < k; ++h) {g[h] = ESKF_LIO::shim::poseFromData(guesses + 16 * h);}
      if (best) {
        const Isometry3d T = icp->alignBest(cloud, *map, g);
        *best = static_cast<int32_t>(icp->lastBestHypothesis());
        if (best_pose) {std::memcpy(best_pose, ESKF_LIO::shim::poseData(T), 16 * sizeof(double));}
        if (iterations) {iterations[0] = icp->lastStats().iterations;}
        if (converged) {converged[0] = icp->lastStats().converged ? 1 : 0;}
      } else {
        const auto all = icp->alignHypotheses(cloud, *map, g);
        for (size_t h = 0; h < all.size(); ++h) {
          if (out_poses) {std::memcpy(out_poses + 16 * h, ESKF_LIO::shim::poseData(all[h].pose), 16 * sizeof(double));}
          if (iterations) {iterations[h] = all[h].iterations;}
          if (converged) {converged[h] = all[h].converged ? 1 : 0;}
          if (final_corr) {final_corr[h] = all[h].finalCorrespondences;}
        }
      }
      if (used_resident) {*used_resident = icp->lastUsedResidentScan() ? 1 : 0;}
    });
}

// One ICP::Evaluation as 31 doubles: points, correspondences (both exact), cost, squaredError, the 27 normal equations.
static void packEvaluation(const ICP::Evaluation & e, double * out)
{
  out[0] = static_cast<double>(e.points);
  out[1] = static_cast<double>(e.correspondences);
  out[2] = e.cost;
  out[3] = e.squaredError;
  for (size_t k = 0; k < 27; ++k) {out[4 + k] = e.normalEquations[k];}
}

// icp->evaluate(cloud, localMap, poses) on a cloud built from the arrays (not resident: one upload); out: k x 31.
int host_icp_evaluate(
  ICP * icp, size_t n, const double * points, const double * covs, const LocalMap * map, size_t k,
  const double * poses, double * out, int32_t * used_resident)
{
  return guarded(
    [&] {
      const PointCloud cloud = makeCloud(n, points, covs);
      std::vector<Isometry3d> g(k);
      for (size_t h = 0; h < k; ++h) {g[h] = ESKF_LIO::shim::poseFromData(poses + 16 * h);}
      const auto all = icp->evaluate(cloud, *map, g);
      for (size_t h = 0; h < all.size(); ++h) {packEvaluation(all[h], out + 31 * h);}
      if (used_resident) {*used_resident = icp->lastUsedResidentScan() ? 1 : 0;}
    });
}

// One ICP::PointReport into the caller's arrays: counts5 = points, matched, counted, negative, notFinite; quantiles as
// asked; the per-point arrays (each optional, `capacity` entries) receive the report's, which the caller trims to points.
static void packPointReport(
  const ICP::PointReport & r, size_t capacity, double * d2, double * sq_error, double * weight, uint8_t * status,
  uint64_t * counts5, double * quantiles)
{
  counts5[0] = r.points; counts5[1] = r.matched; counts5[2] = r.counted; counts5[3] = r.negative; counts5[4] = r.notFinite;
  for (size_t j = 0; j < r.quantiles.size(); ++j) {quantiles[j] = r.quantiles[j];}
  const size_t n = std::min(capacity, r.d2.size());
  if (d2) {std::memcpy(d2, r.d2.data(), n * sizeof(double));}
  if (sq_error) {std::memcpy(sq_error, r.squaredError.data(), n * sizeof(double));}
  if (weight) {std::memcpy(weight, r.weight.data(), n * sizeof(double));}
  if (status) {std::memcpy(status, r.status.data(), n);}
}

// icp->pointReport(cloud, localMap, pose, quantiles, per_point) on a cloud built from the arrays (not resident: one upload).
int host_icp_point_report(
  ICP * icp, size_t n, const double * points, const double * covs, const LocalMap * map, const double pose[16],
  size_t nq, const double * q, int per_point, size_t capacity, double * d2, double * sq_error, double * weight,
  uint8_t * status, uint64_t * counts5, double * quantiles, int32_t * used_resident)
{
  return guarded(
    [&] {
      const PointCloud cloud = makeCloud(n, points, covs);
      const auto r = icp->pointReport(
        cloud, *map, ESKF_LIO::shim::poseFromData(pose), std::vector<double>(q, q + nq), per_point != 0);
      packPointReport(r, capacity, d2, sq_error, weight, status, counts5, quantiles);
      if (used_resident) {*used_resident = icp->lastUsedResidentScan() ? 1 : 0;}
    });
}

// ICP::robustScaleFromQuantile; a refusal is status 1 with the text in host_last_error
int host_icp_robust_scale_from_quantile(double d2_quantile, double factor, double * out)
{
  return guarded([&] {*out = ICP::robustScaleFromQuantile(d2_quantile, factor);});
}

// icp->alignBestByScore(cloud, localMap, guesses): *best the chosen index, best_pose its pose, iterations / converged
// of that hypothesis, evaluation (31 doubles) = icp->lastEvaluation().
int host_icp_align_best_by_score(
  ICP * icp, size_t n, const double * points, const double * covs, const LocalMap * map, size_t k,
  const double * guesses, int32_t * best, double best_pose[16], int32_t * iterations, int32_t * converged,
  double * evaluation)
{
  return guarded(
    [&] {
      const PointCloud cloud = makeCloud(n, points, covs);
      std::vector<Isometry3d> g(k);
      for (size_t h = 0; h < k; ++h) {g[h] = ESKF_LIO::shim::poseFromData(guesses + 16 * h);}
      const Isometry3d T = icp->alignBestByScore(cloud, *map, g);
      *best = static_cast<int32_t>(icp->lastBestHypothesis());
      std::memcpy(best_pose, ESKF_LIO::shim::poseData(T), 16 * sizeof(double));
      if (iterations) {*iterations = icp->lastStats().iterations;}
      if (converged) {*converged = icp->lastStats().converged ? 1 : 0;}
      if (evaluation) {packEvaluation(icp->lastEvaluation(), evaluation);}
    });
}

// Developer aid (tools/probe_eager.py): switch the classes' host-time trace on / off; out (optional) receives
// Trace::Slots seconds followed by Trace::Slots call counts (as doubles) and is then reset.
void host_trace(int enable, double * out)
{
  auto & t = ESKF_LIO::shim::trace();
  if (out) {
    for (int k = 0; k < ESKF_LIO::shim::Trace::Slots; ++k) {
      out[k] = t.seconds[k];
      out[ESKF_LIO::shim::Trace::Slots + k] = static_cast<double>(t.calls[k]);
      t.seconds[k] = 0.0;
      t.calls[k] = 0;
    }
  }
  t.on = enable != 0;
}

// CloudPreprocessor(config) — cloud_preprocessor.voxel_size, sensors.lidar.extrinsics as a 4x4;
// host_copy: 0 = eager (the host cloud holds the prepared scan after process()), 1 = deferred, -1 = the default;
// sampled_check != 0: CloudPreprocessorConfig::residentCheck = Sampled (the default hashes every byte)
CloudPreprocessor * host_preprocessor_create(double voxel_size, const double T_il[16], int host_copy, int sampled_check)
{
  CloudPreprocessor * out = nullptr;
  guarded(
    [&] {
      ESKF_LIO::CloudPreprocessorConfig c;
      c.voxelSize = voxel_size;
      if (T_il) {std::memcpy(c.T_il, T_il, sizeof c.T_il);}
      if (host_copy == 0) {c.hostCopy = ESKF_LIO::CloudPreprocessorConfig::HostCopy::Eager;}
      if (host_copy == 1) {c.hostCopy = ESKF_LIO::CloudPreprocessorConfig::HostCopy::Deferred;}
      if (sampled_check) {c.residentCheck = ESKF_LIO::shim::ResidentCheck::Sampled;}
      out = new CloudPreprocessor(c);
    });
  return out;
}

// ---- one LiDAR frame through the drop-in classes exactly as src/Odometry.cpp:73-87 writes it ----
//   cloudPreprocessor_->process(states, lidarMeas_);                         (:74)
//   transform = kalmanFilter_->update(...) -> icp_->align(*lidar.cloud, localMap, guess)   (:79, ErrorStateKF.cpp:130)
//   localMap_->updateLocalMap(std::move(lidarMeasCopy->cloud), transform);   (:86)
// In three steps so that a caller can time host_frame_run alone (the measurement object is built before).
struct HostFrame
{
  ESKF_LIO::LidarMeasurementPtr meas;
  std::deque<ESKF_LIO::State> states;
  Isometry3d pose;
  int iterations = 0;
  bool usedResident = false;
  size_t corr0 = 0;
};

HostFrame * host_frame_begin(
  size_t n, const double * points, const double * point_time, size_t num_states, const double * states)
{
  HostFrame * f = new HostFrame;
  f->meas = std::make_shared<ESKF_LIO::LidarMeasurement>();
  f->meas->cloud = std::make_shared<PointCloud>();
  f->meas->cloud->points_.resize(n);
  if (n) {std::memcpy(f->meas->cloud->points_.data(), points, n * 24);}
  f->meas->pointTime.assign(point_time, point_time + n);
  f->states.resize(num_states);
  for (size_t s = 0; s < num_states; ++s) {
    f->states[s].timestamp = states[8 * s];
    for (int a = 0; a < 3; ++a) {f->states[s].position(a) = states[8 * s + 1 + a];}
    for (int a = 0; a < 4; ++a) {f->states[s].attitude.c[a] = states[8 * s + 4 + a];}
  }
  return f;
}

// CloudPreprocessor::stage on the frame's measurement (what a lidar callback would do when the sweep arrives): 1 staged
int host_frame_stage(HostFrame * f, const CloudPreprocessor * p)
{
  int staged = 0;
  const int rc = guarded([&] {staged = p->stage(f->meas) ? 1 : 0;});
  return rc == 0 ? staged : -1;
}

// mutate: 0 = the frame as the reference runs it; 1 = the caller edits the prepared cloud between process() and
// align() (its FIRST point moves by 1 mm: an element even the sampled check looks at); 2 = the caller resizes it;
// 3 = the caller edits an element the SAMPLED check never looks at (point 1 of thousands: the default check, which
// hashes every byte, must notice; ResidentCheck::Sampled does not — the documented price of that mode).
// first_frame: process({}, meas) + updateLocalMap(cloud, guess) without align (src/Odometry.cpp:60-61).
// stage_next: a later frame whose sweep "arrives" while this one is being processed: staged (CloudPreprocessor::stage)
// right after this frame's process(), where a lidar callback's thread would be copying beside the device's work.
int host_frame_run(
  HostFrame * f, const CloudPreprocessor * p, ICP * icp, LocalMap * map, const double guess[16], int first_frame,
  int mutate, HostFrame * stage_next, int move_cloud)
{
  return guarded(
    [&] {
      const Isometry3d g = ESKF_LIO::shim::poseFromData(guess);
      if (first_frame) {
        p->process({}, f->meas);
        f->pose = g;
        map->updateLocalMap(f->meas->cloud, g);
        return;
      }
      p->process(f->states, f->meas);
      if (stage_next) {p->stage(stage_next->meas);}
      if (mutate) {ESKF_LIO::shim::materialize(map->context(), *f->meas->cloud);}   // an editor needs the data first
      if (mutate == 1 && !f->meas->cloud->points_.empty()) {f->meas->cloud->points_[0](0) += 1e-3;}
      if (mutate == 3 && f->meas->cloud->points_.size() > 200) {f->meas->cloud->points_[1](0) += 1e-3;}
      if (mutate == 2 && f->meas->cloud->points_.size() > 1) {
        f->meas->cloud->points_.pop_back();
        f->meas->cloud->covariances_.pop_back();
      }
      f->pose = icp->align(*f->meas->cloud, *map, g);
      f->usedResident = icp->lastUsedResidentScan();
      f->iterations = icp->lastStats().iterations;
      f->corr0 = icp->lastStats().correspondenceCounts.empty() ? 0 : icp->lastStats().correspondenceCounts[0];
      // move_cloud: as src/Odometry.cpp:86 hands it over (std::move: the map becomes the cloud's only owner);
      // else a copy of the pointer stays with the frame so that host_frame_end can return the cloud
      if (move_cloud) {map->updateLocalMap(std::move(f->meas->cloud), f->pose);} else {map->updateLocalMap(f->meas->cloud, f->pose);}
    });
}

// process(states, meas) as host_frame_run does it, then icp->alignHypotheses(*meas.cloud, localMap, guesses) on the
// cloud process() just stamped (no updateLocalMap): the fan on the resident scan.  Outputs as host_icp_align_hypotheses.
int host_frame_hypotheses(
  HostFrame * f, const CloudPreprocessor * p, ICP * icp, LocalMap * map, size_t k, const double * guesses,
  double * out_poses, int32_t * iterations, int32_t * converged, uint64_t * final_corr, int32_t * used_resident,
  int32_t * per_launch)
{
  return guarded(
    [&] {
      p->process(f->states, f->meas);
      std::vector<Isometry3d> g(k);
      for (size_t h = 0; h < k; ++h) {g[h] = ESKF_LIO::shim::poseFromData(guesses + 16 * h);}
      const auto all = icp->alignHypotheses(*f->meas->cloud, *map, g);
      for (size_t h = 0; h < all.size(); ++h) {
        if (out_poses) {std::memcpy(out_poses + 16 * h, ESKF_LIO::shim::poseData(all[h].pose), 16 * sizeof(double));}
        if (iterations) {iterations[h] = all[h].iterations;}
        if (converged) {converged[h] = all[h].converged ? 1 : 0;}
        if (final_corr) {final_corr[h] = all[h].finalCorrespondences;}
      }
      if (used_resident) {*used_resident = icp->lastUsedResidentScan() ? 1 : 0;}
      if (per_launch) {*per_launch = icp->lastHypothesesPerLaunch();}
    });
}

// process(states, meas), optionally an edit of the prepared cloud (mutate as host_frame_run), then
// icp->evaluate(*meas.cloud, localMap, poses); out: k x 31 (packEvaluation).
int host_frame_evaluate(
  HostFrame * f, const CloudPreprocessor * p, ICP * icp, LocalMap * map, size_t k, const double * poses, int mutate,
  double * out, int32_t * used_resident)
{
  return guarded(
    [&] {
      p->process(f->states, f->meas);
      if (mutate) {ESKF_LIO::shim::materialize(map->context(), *f->meas->cloud);}
      if (mutate == 1 && !f->meas->cloud->points_.empty()) {f->meas->cloud->points_[0](0) += 1e-3;}
      if (mutate == 2 && f->meas->cloud->points_.size() > 1) {
        f->meas->cloud->points_.pop_back();
        f->meas->cloud->covariances_.pop_back();
      }
      std::vector<Isometry3d> g(k);
      for (size_t h = 0; h < k; ++h) {g[h] = ESKF_LIO::shim::poseFromData(poses + 16 * h);}
      const auto all = icp->evaluate(*f->meas->cloud, *map, g);
      for (size_t h = 0; h < all.size(); ++h) {packEvaluation(all[h], out + 31 * h);}
      if (used_resident) {*used_resident = icp->lastUsedResidentScan() ? 1 : 0;}
    });
}

// process(states, meas), then icp->pointReport(*meas.cloud, localMap, pose, quantiles, per_point) on the cloud process()
// just stamped (no map update): the report of the resident scan.  Outputs as host_icp_point_report.
int host_frame_point_report(
  HostFrame * f, const CloudPreprocessor * p, ICP * icp, LocalMap * map, const double pose[16], size_t nq,
  const double * q, int per_point, size_t capacity, double * d2, double * sq_error, double * weight, uint8_t * status,
  uint64_t * counts5, double * quantiles, int32_t * used_resident)
{
  return guarded(
    [&] {
      p->process(f->states, f->meas);
      const auto r = icp->pointReport(
        *f->meas->cloud, *map, ESKF_LIO::shim::poseFromData(pose), std::vector<double>(q, q + nq), per_point != 0);
      packPointReport(r, capacity, d2, sq_error, weight, status, counts5, quantiles);
      if (used_resident) {*used_resident = icp->lastUsedResidentScan() ? 1 : 0;}
    });
}

// What the frame left: pose, rounds, first round's correspondence count, whether align found the scan resident,
// and the host cloud as it is now (size through *host_points; copied when the arrays are given).
int host_frame_end(
  HostFrame * f, double out_pose[16], int32_t * iterations, int32_t * used_resident, uint64_t * corr0,
  size_t * host_points, size_t capacity, double * points, double * covs)
{
  const int rc = guarded(
    [&] {
      std::memcpy(out_pose, ESKF_LIO::shim::poseData(f->pose), 16 * sizeof(double));
      if (iterations) {*iterations = f->iterations;}
      if (used_resident) {*used_resident = f->usedResident ? 1 : 0;}
      if (corr0) {*corr0 = f->corr0;}
      if (!f->meas->cloud) {                         // moved into the map (host_frame_run with move_cloud)
        if (host_points) {*host_points = 0;}
        return;
      }
      const auto & cloud = *f->meas->cloud;
      if (host_points) {*host_points = cloud.points_.size();}
      if (points && covs && cloud.covariances_.size() == cloud.points_.size() && cloud.points_.size() <= capacity) {
        if (!cloud.points_.empty()) {
          std::memcpy(points, cloud.points_.data(), cloud.points_.size() * 24);
          std::memcpy(covs, cloud.covariances_.data(), cloud.covariances_.size() * 72);
        }
      }
    });
  delete f;
  return rc;
}
void host_preprocessor_destroy(CloudPreprocessor * p) {delete p;}

// preprocessor->voxelDownsampleAndEstimateCovariances(cloud): the cloud is n points (covariances are
// produced); out arrays hold n entries, *kept receives the new size of the cloud.
int host_preprocessor_downsample(
  const CloudPreprocessor * p, size_t n, const double * points, double * out_points, double * out_covs,
  size_t * kept)
{
  return guarded(
    [&] {
      PointCloud cloud;
      cloud.points_.resize(n);
      if (n) {std::memcpy(cloud.points_.data(), points, n * 24);}
      p->voxelDownsampleAndEstimateCovariances(cloud);
      *kept = cloud.points_.size();
      if (*kept) {
        std::memcpy(out_points, cloud.points_.data(), *kept * 24);
        std::memcpy(out_covs, cloud.covariances_.data(), *kept * 72);
      }
    });
}

// preprocessor->process(states, lidarMeas): extrinsic, deskew, down-sampling + covariances.
// states: num_states x 8 (timestamp, position, quaternion x y z w).
int host_preprocessor_process(
  const CloudPreprocessor * p, size_t n, const double * points, const double * point_time,
  size_t num_states, const double * states, double * out_points, double * out_covs, size_t * kept)
{
  return guarded(
    [&] {
      auto meas = std::make_shared<ESKF_LIO::LidarMeasurement>();
      meas->cloud = std::make_shared<PointCloud>();
      meas->cloud->points_.resize(n);
      if (n) {std::memcpy(meas->cloud->points_.data(), points, n * 24);}
      meas->pointTime.assign(point_time, point_time + n);
      std::deque<ESKF_LIO::State> queue(num_states);
      for (size_t s = 0; s < num_states; ++s) {
        queue[s].timestamp = states[8 * s];
        for (int a = 0; a < 3; ++a) {queue[s].position(a) = states[8 * s + 1 + a];}
        for (int a = 0; a < 4; ++a) {queue[s].attitude.c[a] = states[8 * s + 4 + a];}
      }
      p->process(queue, meas);
      ESKF_LIO::shim::materialize(ESKF_LIO::shim::defaultContext(), *meas->cloud);   // a deferred host copy is filled now
      *kept = meas->cloud->points_.size();
      if (*kept) {
        std::memcpy(out_points, meas->cloud->points_.data(), *kept * 24);
        std::memcpy(out_covs, meas->cloud->covariances_.data(), *kept * 72);
      }
      if (!meas->pointTime.empty()) {throw std::runtime_error("process() must clear pointTime");}
    });
}

// The module's own 6x6 solve (csrc/vgicp_math.h, the code the kernels run as their pivoted fallback),
// compiled for the host: lets a CPU-only test pin its operation order against the oracle's LDLT.
// lower21: packed lower triangle row by row; b: right-hand side; x: solution.
void host_math_ldlt6_solve(const double * lower21, const double * b, double * x)
{
  double work[vgicp::kLdltWork];
  vgicp::ldlt6_solve(lower21, b, x, work);
}

// Utils::se3ToSE3 as the module's host math states it -> column-major 4x4.
void host_math_se3_exp(const double * xi, double * out16)
{
  vgicp::Pose T;
  vgicp::se3_exp(xi, T);
  vgicp::pose_to_mat4(T, out16);
}

}  // extern "C"
