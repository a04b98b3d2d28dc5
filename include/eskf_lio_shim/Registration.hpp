// Registration.hpp — drop-in for the reference's include/ESKF_LIO/Registration.hpp +
// src/Registration.cpp: class ESKF_LIO::ICP with the same constructor keys and the same
//   Eigen::Isometry3d align(const PointCloud & cloud, const LocalMap & localMap,
//                           const Eigen::Isometry3d & guess)
// (reference include/ESKF_LIO/Registration.hpp:23-32), so src/ErrorStateKF.cpp:9,130 compiles
// against it unchanged.  align() forwards the raw buffers of the cloud to vgicp_align(): the whole
// loop of src/Registration.cpp:7-35 then runs on the MI355X (see include/vgicp_hip.h).
// Behaviour kept: inputs are not modified; non-convergence only prints "ICP not converged!"
// (src/Registration.cpp:30-32) and still returns the pose.  Behaviour changed on purpose: the
// reference's converged_ member is sticky across calls (Registration.hpp:50, set at
// Registration.cpp:23 and never reset), so after the first converged frame its message can never
// print again; here convergence is per call and readable through lastStats().  A HIP / argument
// error throws std::runtime_error (the reference has no error path at all).
// Added (no counterpart in the reference): alignHypotheses / alignBest register the cloud from a fan of guesses in one
// call (vgicp_hip_batch.h) — for an integrator without a prior, after a stall, or on re-entry into an earlier map.
// evaluate / selectBestByScore / alignBestByScore score poses of a cloud (vgicp_hip_evaluate.h): fitness, inlier RMSE,
// the VGICP objective and the information matrix at a pose, as an Open3D-style RegistrationResult carries them.
// setRobust / the optional keys registration.robust_kernel, robust_scale, gate: a Huber or Cauchy weight and a gate on the
// squared Mahalanobis residual in every round (vgicp_hip_robust.h, which also says in which units).  Absent keys mean
// the reference's plain least squares.
// setPrior / clearPrior / alignWithPrior / posteriorInformation: a Gaussian prior on the pose in every round of the align
// (vgicp_hip_prior.h) — the pose block of the filter's covariance, so that the pose returned is the MAP estimate and
// ErrorStateKF::update can run as an iterated update (INTEGRATION.md has the patch).  No prior set: align() as ever.
// alignCoarseToFine / the optional keys registration.coarse_to_fine.{levels, coarse}: the cloud registered in stages against
// the map's coarser levels (vgicp_hip_map_levels.h; LocalMap::setLevels keeps them), each stage from the pose of the one
// before it — converges from guesses several voxels off, where align() settles in a neighbouring voxel.
// yawFan / setLocate / locate / the optional keys registration.locate.{level, window, stride, yaws, keep}: a pose for a cloud
// whose guess is metres and any yaw off (the first frame against a loaded map, a frame after a stall): a fan of yaws
// scored over a window of whole-voxel shifts on a level of the map (vgicp_hip_map_locate.h), the best few followed up by
// the coarse-to-fine chain, the winner chosen by evaluate().
// pointReport / robustScaleFromQuantile: a cloud at a pose, point by point (vgicp_hip_points.h) — matched or not, |e|^2,
// d^2, the weight this ICP's robust settings give the point — and order statistics of d^2 to choose a scale or gate by.
#ifndef ESKF_LIO_SHIM_REGISTRATION_HPP_
#define ESKF_LIO_SHIM_REGISTRATION_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "LocalMap.hpp"
#include "../vgicp_hip_batch.h"
#include "../vgicp_hip_evaluate.h"
#include "../vgicp_hip_robust.h"
#include "../vgicp_hip_prior.h"
#include "../vgicp_hip_points.h"
#include "../vgicp_hip_map_levels.h"
#include "../vgicp_hip_map_locate.h"

// referenced weakly, as LocalMap.hpp references the raw-point store's entry points: a program that links a stand-in of
// the C ABI without them, or that does not link libvgicp_hip_prior.so beside libvgicp_hip.so, still links, and
// ICP::setPrior then says so
#pragma weak vgicp_set_pose_prior
#pragma weak vgicp_pose_prior_chart
// ... and libvgicp_hip_points.so's: ICP::pointReport says so
#pragma weak vgicp_points_resident
// ... and libvgicp_hip_map_levels.so's: ICP::alignCoarseToFine says so
#pragma weak vgicp_align_resident_levels
// ... and libvgicp_hip_map_locate.so's: ICP::locate says so
#pragma weak vgicp_locate_resident

namespace ESKF_LIO
{

// A 6 x 6 information matrix in the filter's chart [t - t0; Log(R0^T R)], column-major behind data().
#if defined(ESKF_LIO_SHIM_NATIVE_TYPES)
using Matrix6d = Eigen::Matrix<double, 6, 6>;
#else
struct Matrix6d
{
  double m[36];
  static Matrix6d Zero()
  {
    Matrix6d z;
    for (double & v : z.m) {v = 0.0;}
    return z;
  }
  const double * data() const {return m;}
  double * data() {return m;}
  double & operator()(int r, int c) {return m[r + 6 * c];}
  double operator()(int r, int c) const {return m[r + 6 * c];}
};
#endif

// What ICP::locate searches and follows up (ICP::setLocate; registration.locate.* in the YAML file).
struct LocateOptions
{
  int level = 3;                            // the level of the map the fan is scored on
  std::array<int, 3> window{{4, 4, 1}};     // half-widths of the window of shifts, in voxels of that level
  unsigned stride = 1;                      // every stride-th point of the cloud takes part in the search
  int yaws = 64;                            // poses of the yaw fan, at most VGICP_LOCATE_MAX_POSES
  int keep = 4;                             // candidates followed up by the chain, at most 8
  std::vector<int> schedule;                // of that chain; empty: the ICP's coarse-to-fine schedule
};

// The keys ICP's YAML constructor reads (config/hilti_config.yaml:50-53).
struct RegistrationConfig
{
  int maxIteration = 100;
  double translationSquaredThreshold = 1.0e-6;
  double cosineThreshold = 0.9999;
  int chunkIterations = 0;  // vgicp_params.chunk_iterations; 0 = library default
  // robust rounds (vgicp_hip_robust.h; not in the reference's file): registration.robust_kernel / robust_scale / gate
  int robustKernel = VGICP_ROBUST_NONE;
  double robustScale = 1.0;   // c, in the library's regularised units (~0.1, not ~3)
  double robustGate = 0.0;    // gate on d^2; 0 = none
  // coarse to fine (vgicp_hip_map_levels.h; not in the reference's file): registration.coarse_to_fine.levels, the level of
  // every stage, e.g. [3, 2, 1, 0], and registration.coarse_to_fine.coarse.{max_iteration, translation_sq_threshold,
  // cosine_threshold} for every stage but the last, which takes the three values above
  std::vector<int> coarseToFineLevels;
  int coarseMaxIteration = 30;
  double coarseTranslationSquaredThreshold = 1.0e-4;
  double coarseCosineThreshold = 0.999;
  // locate (vgicp_hip_map_locate.h; not in the reference's file): registration.locate.{level, window, stride, yaws, keep}
  LocateOptions locate;

  // registration.robust_kernel: none | huber | cauchy
  static int robustKernelFromName(const std::string & name)
  {
    if (name == "none") {return VGICP_ROBUST_NONE;}
    if (name == "huber") {return VGICP_ROBUST_HUBER;}
    if (name == "cauchy") {return VGICP_ROBUST_CAUCHY;}
    throw std::invalid_argument("registration.robust_kernel must be none, huber or cauchy, not '" + name + "'");
  }
};

class ICP
{
public:
  using PointVector = typename std::vector<Vector3d>;
  using CovarianceVector = typename std::vector<Matrix3d>;
  using Correspondence = typename std::tuple<PointVector, CovarianceVector, PointVector,
      CovarianceVector>;

  struct Stats
  {
    int iterations = 0;
    bool converged = false;
    double seconds = 0.0;
    double deviceSeconds = 0.0;
    std::vector<uint64_t> correspondenceCounts;
  };

  explicit ICP(const RegistrationConfig & config)
  : maxIteration_(config.maxIteration)
    , translationSquaredThreshold_(config.translationSquaredThreshold)
    , cosineThreshold_(config.cosineThreshold)
    , chunkIterations_(config.chunkIterations)
  {
    setRobust(config.robustKernel, config.robustScale, config.robustGate);
    setCoarseToFine(
      config.coarseToFineLevels, config.coarseMaxIteration, config.coarseTranslationSquaredThreshold,
      config.coarseCosineThreshold);
    setLocate(config.locate);
  }

#if defined(ESKF_LIO_SHIM_HAVE_YAML)
  ICP(const YAML::Node & config)
  : maxIteration_(config["registration"]["max_iteration"].as<int>())
    , translationSquaredThreshold_(config["registration"]["translation_sq_threshold"].as<double>())
    , cosineThreshold_(config["registration"]["cosine_threshold"].as<double>())
  {
    // optional keys, not in the reference's file; absent = the reference's plain least squares
    const YAML::Node reg = config["registration"];
    RegistrationConfig c;
    if (reg["robust_kernel"].IsDefined()) {
      c.robustKernel = RegistrationConfig::robustKernelFromName(reg["robust_kernel"].as<std::string>());
    }
    if (reg["robust_scale"].IsDefined()) {c.robustScale = reg["robust_scale"].as<double>();}
    if (reg["gate"].IsDefined()) {c.robustGate = reg["gate"].as<double>();}
    setRobust(c.robustKernel, c.robustScale, c.robustGate);
    if (reg["coarse_to_fine"].IsDefined()) {
      const YAML::Node ctf = reg["coarse_to_fine"];
      if (ctf["levels"].IsDefined()) {c.coarseToFineLevels = ctf["levels"].as<std::vector<int>>();}
      const YAML::Node coarse = ctf["coarse"];
      if (coarse.IsDefined()) {
        if (coarse["max_iteration"].IsDefined()) {c.coarseMaxIteration = coarse["max_iteration"].as<int>();}
        if (coarse["translation_sq_threshold"].IsDefined()) {
          c.coarseTranslationSquaredThreshold = coarse["translation_sq_threshold"].as<double>();
        }
        if (coarse["cosine_threshold"].IsDefined()) {c.coarseCosineThreshold = coarse["cosine_threshold"].as<double>();}
      }
      setCoarseToFine(
        c.coarseToFineLevels, c.coarseMaxIteration, c.coarseTranslationSquaredThreshold, c.coarseCosineThreshold);
    }
    if (reg["locate"].IsDefined()) {
      const YAML::Node loc = reg["locate"];
      // an empty window and a stride, yaws or keep of 0 mean the default, as chunk_iterations: 0 does
      if (loc["level"].IsDefined()) {c.locate.level = loc["level"].as<int>();}
      if (loc["window"].IsDefined()) {
        const std::vector<int> w = loc["window"].as<std::vector<int>>();
        if (!w.empty() && w.size() != 3) {
          throw std::invalid_argument("registration.locate.window must have three half-widths");
        }
        if (!w.empty()) {c.locate.window = {{w[0], w[1], w[2]}};}
      }
      if (loc["stride"].IsDefined()) {
        const int stride = loc["stride"].as<int>();
        if (stride < 0) {throw std::invalid_argument("registration.locate.stride must be >= 1");}
        if (stride > 0) {c.locate.stride = static_cast<unsigned>(stride);}
      }
      if (loc["yaws"].IsDefined() && loc["yaws"].as<int>() != 0) {c.locate.yaws = loc["yaws"].as<int>();}
      if (loc["keep"].IsDefined() && loc["keep"].as<int>() != 0) {c.locate.keep = loc["keep"].as<int>();}
      setLocate(c.locate);
    }
  }
#endif

  // The schedule alignCoarseToFine(cloud, map, guess) walks and what every stage but the last stops by (the last stage
  // takes this ICP's own three values, as align() does).  Throws std::invalid_argument for anything the library would
  // refuse, and changes nothing then.  An empty schedule: alignCoarseToFine without one is align().
  void setCoarseToFine(
    const std::vector<int> & levels, int coarseMaxIteration = 30, double coarseTranslationSquaredThreshold = 1.0e-4,
    double coarseCosineThreshold = 0.999)
  {
    checkSchedule(levels);
    if (coarseMaxIteration < 0) {throw std::invalid_argument("ICP::setCoarseToFine: coarse max_iteration < 0");}
    schedule_ = levels;
    coarseMaxIteration_ = coarseMaxIteration;
    coarseTranslationSquaredThreshold_ = coarseTranslationSquaredThreshold;
    coarseCosineThreshold_ = coarseCosineThreshold;
  }
  const std::vector<int> & coarseToFineLevels() const {return schedule_;}

  // One stage of the last alignCoarseToFine.
  struct StageStats
  {
    int level = 0;
    Stats stats;
  };

  // Registers `cloud` in stages (vgicp_align_resident_levels): stage i against level schedule[i] of the map, from the pose
  // stage i - 1 returned (stage 0: from guess); every stage but the last with the coarse thresholds, the last with this
  // ICP's own.  The map must keep the levels the schedule names (LocalMap::setLevels; the YAML constructors of both classes
  // read the same key).  The cloud is the resident scan when it still is what CloudPreprocessor::process left on the
  // device (as alignHypotheses decides it), else ONE upload of it.  Robust settings and prior apply to every stage.
  // lastStats() describes the last stage, lastStages() all of them.
  Isometry3d alignCoarseToFine(
    const PointCloud & cloud, const LocalMap & localMap, const Isometry3d & guess, const std::vector<int> & schedule)
  {
    checkSchedule(schedule);
    if (schedule.empty()) {throw std::invalid_argument("ICP::alignCoarseToFine: the schedule is empty");}
    if (!vgicp_align_resident_levels) {
      throw std::runtime_error(
              "ICP::alignCoarseToFine: the linked vgicp module has no vgicp_align_resident_levels (libvgicp_hip_map_levels.so)");
    }
    vgicp_ctx * ctx = localMap.context();
    applyRobust(ctx);
    applyPrior(ctx);
    lastUsedResidentScan_ = residentScanOrUpload(ctx, cloud, "alignCoarseToFine");
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    return chainResidentScan(ctx, guess, schedule);
  }
  // ... with the schedule this ICP was given (setCoarseToFine, registration.coarse_to_fine.levels); none: align()
  Isometry3d alignCoarseToFine(const PointCloud & cloud, const LocalMap & localMap, const Isometry3d & guess)
  {
    return schedule_.empty() ? align(cloud, localMap, guess) : alignCoarseToFine(cloud, localMap, guess, schedule_);
  }
  const std::vector<StageStats> & lastStages() const {return lastStages_;}          // of the last alignCoarseToFine()

  // Where is this piece of `source` in `target`?  (Loop closure, the merge of two sessions, the re-entry into a loaded
  // map with more than one sweep.)  The voxels of source within `radius` of anchor's translation become target's
  // resident scan in the frame anchor^-1 (LocalMap::scanFromMap; minCount and level as there), i.e. as the cloud a sensor
  // at `anchor` would have prepared, and are registered on target from `guess`, the anchor's pose in target's map as far
  // as it is known (the anchor itself when the two maps are believed to share a frame) — through the coarse-to-fine
  // chain when this ICP has a schedule (setCoarseToFine; target must keep the levels), else by one align.  Returns the
  // anchor's pose in target's map; lastStats() / lastStages() describe the registration, lastSubmap() the selection.
  // Throws std::runtime_error when nothing was selected.
  Isometry3d alignSubmap(
    LocalMap & source, LocalMap & target, const Isometry3d & anchor, double radius, const Isometry3d & guess,
    size_t minCount = 0, int level = 0)
  {
    lastSubmap_ = target.scanFromMap(source, anchor.translation(), radius, anchor.inverse(), minCount, level);
    if (lastSubmap_.points == 0) {throw std::runtime_error("ICP::alignSubmap: no voxel of the source was selected");}
    vgicp_ctx * ctx = target.context();
    applyRobust(ctx);
    applyPrior(ctx);
    lastUsedResidentScan_ = true;
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    if (!schedule_.empty()) {
      if (!vgicp_align_resident_levels) {
        throw std::runtime_error(
                "ICP::alignSubmap: the linked vgicp module has no vgicp_align_resident_levels (libvgicp_hip_map_levels.so)");
      }
      return chainResidentScan(ctx, guess, schedule_);
    }
    const vgicp_params params = paramsOf();
    std::vector<uint64_t> counts(static_cast<size_t>(maxIteration_ > 0 ? maxIteration_ : 1), 0);
    vgicp_stats stats{};
    stats.corr_count = counts.data();
    double pose[16];
    const int rc = vgicp_align_resident(ctx, shim::poseData(guess), &params, pose, &stats);
    if (rc != VGICP_OK && rc != VGICP_ERR_DEGENERATE) {shim::check(ctx, rc, "vgicp_align_resident");}
    lastStats_.iterations = stats.iterations;
    lastStats_.converged = stats.converged != 0;
    lastStats_.seconds = stats.seconds;
    lastStats_.deviceSeconds = stats.device_seconds;
    counts.resize(static_cast<size_t>(stats.iterations));
    lastStats_.correspondenceCounts = counts;
    if (!lastStats_.converged) {
      std::cout << "ICP not converged!\n";
    }
    return shim::poseFromData(pose);
  }
  const LocalMap::SubmapStats & lastSubmap() const {return lastSubmap_;}          // of the last alignSubmap()

  // The robust round of every later align / alignHypotheses of this ICP (vgicp_hip_robust.h): kind = VGICP_ROBUST_NONE,
  // _HUBER or _CAUCHY, its scale c, and the gate on the squared Mahalanobis residual (0 = none), in the library's
  // regularised units.  The library takes millionths: scale and gate are rounded to them.  Throws std::invalid_argument
  // for anything the library would refuse, and changes nothing then.  While a kernel or a gate is set,
  // alignHypotheses registers its guesses one by one (lastHypothesesPerLaunch() == 1) and evaluate() still scores the
  // plain objective.
  void setRobust(int kind, double scale, double gate)
  {
    if (kind != VGICP_ROBUST_NONE && kind != VGICP_ROBUST_HUBER && kind != VGICP_ROBUST_CAUCHY) {
      throw std::invalid_argument("ICP::setRobust: kind must be VGICP_ROBUST_NONE, _HUBER or _CAUCHY");
    }
    const double scaleMicro = std::round(scale * 1e6), gateMicro = std::round(gate * 1e6);
    if (!(scaleMicro >= 1.0 && scaleMicro <= 2147483647.0)) {
      throw std::invalid_argument("ICP::setRobust: scale must be in [1e-6, 2147.48]");
    }
    if (!(gateMicro >= 0.0 && gateMicro <= 2147483647.0)) {
      throw std::invalid_argument("ICP::setRobust: gate must be in [0, 2147.48]");
    }
    robustKernel_ = kind;
    robustScaleMicro_ = static_cast<int>(scaleMicro);
    robustGateMicro_ = static_cast<int>(gateMicro);
  }
  int robustKernel() const {return robustKernel_;}
  double robustScale() const {return robustScaleMicro_ / 1000000.0;}   // as the library uses it
  double robustGate() const {return robustGateMicro_ / 1000000.0;}

  // A Gaussian prior on the pose for every later align / alignHypotheses of this ICP (vgicp_hip_prior.h): the pose
  // priorPose and a symmetric positive semi-definite information matrix in the chart [t - t0; Log(R0^T R)] (translation
  // first) — the inverse of the pose block of the filter's P.  The library checks the values at the next align and
  // refuses bad ones there (std::runtime_error with its text).  An all-zero information is no prior.
  void setPrior(const Isometry3d & priorPose, const Matrix6d & information)
  {
    const double * p = shim::poseData(priorPose);
    for (int k = 0; k < 16; ++k) {priorPose_[static_cast<size_t>(k)] = p[k];}
    for (int k = 0; k < 36; ++k) {priorInformation_[static_cast<size_t>(k)] = information.data()[k];}
    priorOn_ = true;
  }
  void clearPrior() {priorOn_ = false;}
  bool hasPrior() const {return priorOn_;}

  // setPrior(guess, priorInformation), align, clearPrior: the MAP pose of the cloud given the filter's pose `guess` with
  // information priorInformation.  Leaves no prior behind, neither on this ICP nor on the map's context, and keeps what
  // posteriorInformation() returns.
  Isometry3d alignWithPrior(
    const PointCloud & cloud, const LocalMap & localMap, const Isometry3d & guess, const Matrix6d & priorInformation)
  {
    setPrior(guess, priorInformation);
    struct Clear
    {
      ICP * self;
      vgicp_ctx * ctx;
      ~Clear()
      {
        self->clearPrior();
        if (vgicp_set_pose_prior) {(void)vgicp_set_pose_prior(ctx, nullptr, nullptr);}
      }
    } clear{this, localMap.context()};
    const Isometry3d pose = align(cloud, localMap, guess);
    // the data's information at the returned pose (the align left the cloud resident), carried from the chart of the
    // normal equations into the filter's: G^-T A G^-1, plus the prior's
    const std::vector<Evaluation> at = evaluateResidentScan(localMap.context(), {pose});
    const std::array<double, 36> A = at[0].information();
    double G[36], Ginv[36];
    shim::check(localMap.context(), vgicp_pose_prior_chart(shim::poseData(guess), shim::poseData(pose), nullptr, G),
      "vgicp_pose_prior_chart");
    if (!invert6(G, Ginv)) {throw std::runtime_error("ICP::alignWithPrior: the chart's Jacobian is singular");}
    double AG[36];
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) {
        double v = 0.0;
        for (int k = 0; k < 6; ++k) {v += A[static_cast<size_t>(r + 6 * k)] * Ginv[k + 6 * c];}
        AG[r + 6 * c] = v;
      }
    }
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) {
        double v = 0.0;
        for (int k = 0; k < 6; ++k) {v += Ginv[k + 6 * r] * AG[k + 6 * c];}
        posterior_.data()[r + 6 * c] = v + priorInformation.data()[r + 6 * c];
      }
    }
    return pose;
  }

  // Of the last alignWithPrior: G^-T A G^-1 + priorInformation in the filter's chart — A the data's information at the
  // returned pose (evaluate), G the chart's Jacobian there (vgicp_pose_prior_chart).  Its inverse is the covariance of
  // the returned pose.
  Matrix6d posteriorInformation() const {return posterior_;}

  Isometry3d align(const PointCloud & cloud, const LocalMap & localMap, const Isometry3d & guess)
  {
    vgicp_ctx * ctx = localMap.context();
    applyRobust(ctx);
    applyPrior(ctx);
    const vgicp_params params = paramsOf();
    std::vector<uint64_t> counts(static_cast<size_t>(maxIteration_ > 0 ? maxIteration_ : 1), 0);
    vgicp_stats stats{};
    stats.corr_count = counts.data();
    double pose[16];
    // The cloud CloudPreprocessor::process just prepared is resident on the device already (src/Odometry.cpp:74 ->
    // src/ErrorStateKF.cpp:130 hand it over untouched): no second upload of its 96 bytes per point, and the frame's
    // one synchronisation is this call's.  Any other cloud — or that one after somebody changed it — goes up as it is.
    int rc = VGICP_OK;
    shim::ResidentStamp * resident = nullptr;
    bool done = false;
    {
      shim::TraceScope ts(shim::Trace::AlignVerify);
      resident = shim::residentIdentityOf(ctx, cloud);
    }
    shim::HashCrew & crew = shim::HashCrew::instance();
    if (resident && !resident->sampled && crew.helpers() > 0 &&
      cloud.points_.size() * (sizeof(Vector3d) + sizeof(Matrix3d)) >= (256u << 10))
    {
      // The full-hash check of a large cloud and the registration at the same time: helper threads read the host cloud
      // while this thread waits for the device, which registers its own copy.  The result counts only if the hash then
      // matches the stamp; a cloud edited since is registered again below from the host data, as the reference would
      // (vgicp_align_resident changes neither the resident scan nor the map).
      shim::FullHashJob job;
      shim::planFullHash(cloud, job, crew.helpers());
      crew.begin(job.chunks, job.count);
      {
        shim::TraceScope tsCall(shim::Trace::AlignCall);
        rc = vgicp_align_resident(ctx, shim::poseData(guess), &params, pose, &stats);
      }
      {
        shim::TraceScope ts(shim::Trace::AlignVerify);
        crew.finish();
        done = shim::foldFullHash(job) == resident->hash;
      }
      if (!done) {resident = nullptr;}
    } else if (resident) {
      shim::TraceScope ts(shim::Trace::AlignVerify);
      if (resident->hash != shim::sampleHash(cloud, resident->sampled)) {resident = nullptr;}
    }
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    if (done) {
      lastUsedResidentScan_ = true;
    } else if (resident) {
      rc = vgicp_align_resident(ctx, shim::poseData(guess), &params, pose, &stats);
      lastUsedResidentScan_ = true;
    } else {
      const size_t n = pointsWithCovariances(cloud, "align");
      const double * pts = n ? cloud.points_.data()->data() : nullptr;
      const double * covs = n ? cloud.covariances_.data()->data() : nullptr;
      rc = vgicp_align(ctx, n, pts, covs, shim::poseData(guess), &params, pose, &stats);
      lastUsedResidentScan_ = false;
    }
    if (rc != VGICP_OK && rc != VGICP_ERR_DEGENERATE) {shim::check(ctx, rc, "vgicp_align");}

    lastStats_.iterations = stats.iterations;
    lastStats_.converged = stats.converged != 0;
    lastStats_.seconds = stats.seconds;
    lastStats_.deviceSeconds = stats.device_seconds;
    counts.resize(static_cast<size_t>(stats.iterations));
    lastStats_.correspondenceCounts = counts;
    if (!lastStats_.converged) {
      std::cout << "ICP not converged!\n";
    }
    return shim::poseFromData(pose);
  }

  // One registration of a fan: what align() would have returned and reported for that guess.
  struct Hypothesis
  {
    Isometry3d pose;
    bool converged = false;
    int iterations = 0;
    uint64_t finalCorrespondences = 0;   // correspondences of the last round
  };

  // Registers `cloud` from every guess (at most VGICP_BATCH_MAX) in one call of vgicp_align_resident_batch: the resident
  // scan when the cloud still is what CloudPreprocessor::process left on the device (the stamp and the hash of the host
  // data say so, as in align()), else ONE upload of the cloud.  Each result is bit for bit align()'s for that guess.
  std::vector<Hypothesis> alignHypotheses(
    const PointCloud & cloud, const LocalMap & localMap, const std::vector<Isometry3d> & guesses)
  {
    std::vector<Hypothesis> out;
    const size_t k = guesses.size();
    if (k == 0) {return out;}
    if (k > static_cast<size_t>(VGICP_BATCH_MAX)) {
      throw std::runtime_error("ICP::alignHypotheses: more than VGICP_BATCH_MAX guesses");
    }
    vgicp_ctx * ctx = localMap.context();
    applyRobust(ctx);
    applyPrior(ctx);
    const vgicp_params params = paramsOf();
    lastUsedResidentScan_ = residentScanOrUpload(ctx, cloud, "alignHypotheses");
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    const size_t rounds = static_cast<size_t>(maxIteration_ > 0 ? maxIteration_ : 0);
    std::vector<double> in(16 * k), poses(16 * k);
    for (size_t h = 0; h < k; ++h) {
      const double * g = shim::poseData(guesses[h]);
      for (int e = 0; e < 16; ++e) {in[16 * h + e] = g[e];}
    }
    std::vector<int32_t> status(k, 0), iterations(k, 0), converged(k, 0);
    fanCounts_.assign(k * rounds + 1, 0);
    fanRounds_ = rounds;
    vgicp_batch_stats stats{};
    stats.status = status.data();
    stats.iterations = iterations.data();
    stats.converged = converged.data();
    stats.corr_count = fanCounts_.data();
    // (a hypothesis whose pose is not finite comes back in status[], as align() returns such a pose: no throw)
    shim::check(ctx, vgicp_align_resident_batch(ctx, k, in.data(), &params, poses.data(), &stats),
      "vgicp_align_resident_batch");
    fanSeconds_ = stats.seconds;
    fanDeviceSeconds_ = stats.device_seconds;
    lastHypothesesPerLaunch_ = stats.hypotheses_per_launch;
    out.resize(k);
    for (size_t h = 0; h < k; ++h) {
      out[h].pose = shim::poseFromData(poses.data() + 16 * h);
      out[h].converged = converged[h] != 0;
      out[h].iterations = iterations[h];
      out[h].finalCorrespondences = iterations[h] > 0 ? fanCounts_[h * rounds + static_cast<size_t>(iterations[h]) - 1] : 0;
    }
    return out;
  }

  // Which hypothesis of a fan to keep: the one with the most correspondences in its last round; a converged one goes
  // before one that is not, ties go to the lower index.  (A fan that straddles two basins is told apart by that count
  // alone: the wrong basin matches far fewer points.)  hypotheses must not be empty.
  static size_t selectBest(const std::vector<Hypothesis> & hypotheses)
  {
    size_t best = 0;
    for (size_t h = 1; h < hypotheses.size(); ++h) {
      const Hypothesis & a = hypotheses[h];
      const Hypothesis & b = hypotheses[best];
      if ((a.converged && !b.converged) ||
        (a.converged == b.converged && a.finalCorrespondences > b.finalCorrespondences))
      {
        best = h;
      }
    }
    return best;
  }

  // alignHypotheses, then the pose of selectBest's choice; lastStats() describes that hypothesis, as after align().
  Isometry3d alignBest(
    const PointCloud & cloud, const LocalMap & localMap, const std::vector<Isometry3d> & guesses)
  {
    if (guesses.empty()) {throw std::runtime_error("ICP::alignBest: no guess");}
    const std::vector<Hypothesis> all = alignHypotheses(cloud, localMap, guesses);
    const size_t best = selectBest(all);
    lastBest_ = best;
    lastStats_.iterations = all[best].iterations;
    lastStats_.converged = all[best].converged;
    lastStats_.seconds = fanSeconds_;
    lastStats_.deviceSeconds = fanDeviceSeconds_;
    lastStats_.correspondenceCounts.assign(
      fanCounts_.begin() + static_cast<std::ptrdiff_t>(best * fanRounds_),
      fanCounts_.begin() + static_cast<std::ptrdiff_t>(best * fanRounds_ + static_cast<size_t>(all[best].iterations)));
    if (!lastStats_.converged) {
      std::cout << "ICP not converged!\n";
    }
    return all[best].pose;
  }

  // A pose of a cloud, scored against the map (one vgicp_evaluation).
  struct Evaluation
  {
    uint64_t points = 0;            // of the cloud
    uint64_t correspondences = 0;   // points whose voxel is in the map at the pose
    double cost = 0.0;              // sum over the correspondences of e^T (R C R^T + C_voxel)^-1 e: ICP::align's objective
    double squaredError = 0.0;      // sum over the correspondences of |e|^2
    std::array<double, 27> normalEquations{};   // packed as vgicp_evaluation::normal_eq

    double fitness() const {return points ? static_cast<double>(correspondences) / static_cast<double>(points) : 0.0;}
    double inlierRmse() const
    {
      return correspondences ? std::sqrt(squaredError / static_cast<double>(correspondences)) : 0.0;
    }
    // J^T Sigma^-1 J at the pose, 6 x 6 (symmetric; translation first, then rotation, as the normal equations): the
    // information matrix of the registration, for an integrator that wants a pose covariance instead of a fixed one.
    std::array<double, 36> information() const
    {
      std::array<double, 36> m{};
      int k = 0;
      for (int r = 0; r < 6; ++r) {
        for (int c = 0; c <= r; ++c, ++k) {m[r + 6 * c] = m[c + 6 * r] = normalEquations[static_cast<size_t>(k)];}
      }
      return m;
    }
    // The objective with every point that found no voxel charged missPenalty, like a rejected measurement.  The default
    // is the 0.99 quantile of chi-squared with 3 degrees of freedom: the cost at which a matched point would itself be
    // called an outlier.
    double score(double missPenalty = 11.345) const
    {
      return cost + missPenalty * static_cast<double>(points - correspondences);
    }
  };

  // Scores `cloud` at every pose (at most VGICP_EVAL_MAX) in one call of vgicp_evaluate_resident: the resident scan when
  // the cloud still is what CloudPreprocessor::process left on the device (as alignHypotheses decides it), else ONE
  // upload of the cloud.  Changes neither the map nor what a later align returns.
  std::vector<Evaluation> evaluate(
    const PointCloud & cloud, const LocalMap & localMap, const std::vector<Isometry3d> & poses)
  {
    std::vector<Evaluation> out;
    const size_t k = poses.size();
    if (k == 0) {return out;}
    if (k > static_cast<size_t>(VGICP_EVAL_MAX)) {
      throw std::runtime_error("ICP::evaluate: more than VGICP_EVAL_MAX poses");
    }
    vgicp_ctx * ctx = localMap.context();
    lastUsedResidentScan_ = residentScanOrUpload(ctx, cloud, "evaluate");
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    return evaluateResidentScan(ctx, poses);
  }

  // ---- locate (vgicp_hip_map_locate.h): a pose for a cloud that has no guess an align converges from ----
  using LocateOptions = ESKF_LIO::LocateOptions;

  // count poses about the sensor's position at `guess`: pose j is [Rz(2 pi j / count) R_guess | t_guess], a rotation about
  // the world's z through that position.
  static std::vector<Isometry3d> yawFan(const Isometry3d & guess, int count)
  {
    if (count < 1) {throw std::invalid_argument("ICP::yawFan: count < 1");}
    const double * g = shim::poseData(guess);
    std::vector<Isometry3d> fan;
    fan.reserve(static_cast<size_t>(count));
    for (int j = 0; j < count; ++j) {
      const double a = 2.0 * 3.14159265358979323846 * static_cast<double>(j) / static_cast<double>(count);
      const double c = std::cos(a), s = std::sin(a);
      double m[16];
      for (int e = 0; e < 16; ++e) {m[e] = g[e];}
      for (int col = 0; col < 3; ++col) {          // Rz(a) R: rows x and y of every column of R
        m[0 + 4 * col] = c * g[0 + 4 * col] - s * g[1 + 4 * col];
        m[1 + 4 * col] = s * g[0 + 4 * col] + c * g[1 + 4 * col];
      }
      fan.push_back(shim::poseFromData(m));
    }
    return fan;
  }

  // What locate() searches and follows up.  Throws std::invalid_argument for anything the library would refuse, and
  // changes nothing then.  An empty schedule means this ICP's coarse-to-fine schedule (setCoarseToFine).
  void setLocate(const LocateOptions & options)
  {
    if (options.level < 0 || options.level > VGICP_LEVELS_MAX) {
      throw std::invalid_argument("ICP::setLocate: level must be 0 .. VGICP_LEVELS_MAX");
    }
    long cells = 1;
    for (const int w : options.window) {
      if (w < 0 || w > VGICP_LOCATE_MAX_HALF_WIDTH) {
        throw std::invalid_argument("ICP::setLocate: a half-width of the window must be 0 .. VGICP_LOCATE_MAX_HALF_WIDTH");
      }
      cells *= 2 * w + 1;
    }
    if (cells > VGICP_LOCATE_MAX_CELLS) {
      throw std::invalid_argument("ICP::setLocate: the window has more than VGICP_LOCATE_MAX_CELLS cells");
    }
    if (options.stride < 1) {throw std::invalid_argument("ICP::setLocate: stride < 1");}
    if (options.yaws < 1 || options.yaws > VGICP_LOCATE_MAX_POSES) {
      throw std::invalid_argument("ICP::setLocate: yaws must be 1 .. VGICP_LOCATE_MAX_POSES");
    }
    if (options.keep < 1 || options.keep > kLocateKeepMax) {throw std::invalid_argument("ICP::setLocate: keep must be 1 .. 8");}
    checkSchedule(options.schedule);
    locate_ = options;
  }
  const LocateOptions & locateOptions() const {return locate_;}

  // One candidate of the last locate(): a pose of the fan, what vgicp_locate_resident found for it, where the chain from
  // there ended and how the cloud scores at that end.
  struct LocateCandidate
  {
    int poseIndex = 0;               // in the yaw fan
    uint32_t hits = 0;               // of the pose's best cell
    std::array<int, 3> offset{};     // that cell's shift, in voxels of the level
    Isometry3d start;                // the fan's pose moved by the shift: where the chain started
    Isometry3d pose;                 // where it ended
    Evaluation evaluation;           // of the cloud at `pose`
  };

  // Finds a pose for `cloud` from a guess that may be metres and any yaw off: ONE call of vgicp_locate_resident on the yaw
  // fan about `guess`; the poses ranked by the hits of their best cell (descending, ties to the lower index); the first
  // `keep` of them followed up by the coarse-to-fine chain (alignCoarseToFine's stages) from the located pose; the ends
  // scored by one evaluate; the one with the most correspondences (ties: the lower cost, then the better rank) returned.
  // The map must keep the level searched and the levels of the schedule (LocalMap::setLevels).  The cloud is the
  // resident scan when it still is what CloudPreprocessor::process left on the device, else ONE upload of it.
  // lastLocation() lists the candidates in rank order, lastLocationWinner() the index of the one returned; lastStats()
  // and lastStages() describe the last chain run, lastEvaluation() the winner.
  Isometry3d locate(const PointCloud & cloud, const LocalMap & localMap, const Isometry3d & guess)
  {
    if (!vgicp_locate_resident) {
      throw std::runtime_error(
              "ICP::locate: the linked vgicp module has no vgicp_locate_resident (libvgicp_hip_map_locate.so)");
    }
    if (!vgicp_align_resident_levels) {
      throw std::runtime_error(
              "ICP::locate: the linked vgicp module has no vgicp_align_resident_levels (libvgicp_hip_map_levels.so)");
    }
    const std::vector<int> & schedule = locate_.schedule.empty() ? schedule_ : locate_.schedule;
    if (schedule.empty()) {
      throw std::invalid_argument("ICP::locate: no schedule (LocateOptions::schedule or setCoarseToFine)");
    }
    vgicp_ctx * ctx = localMap.context();
    applyRobust(ctx);
    applyPrior(ctx);
    lastUsedResidentScan_ = residentScanOrUpload(ctx, cloud, "locate");
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    const std::vector<Isometry3d> fan = yawFan(guess, locate_.yaws);
    const size_t k = fan.size();
    std::vector<double> in(16 * k);
    for (size_t h = 0; h < k; ++h) {
      const double * g = shim::poseData(fan[h]);
      for (int e = 0; e < 16; ++e) {in[16 * h + static_cast<size_t>(e)] = g[e];}
    }
    vgicp_locate_params params{};
    params.level = locate_.level;
    for (size_t a = 0; a < 3; ++a) {params.window[a] = locate_.window[a];}
    params.stride = locate_.stride;
    std::vector<vgicp_locate_best> best(k);
    shim::check(
      ctx, vgicp_locate_resident(ctx, in.data(), k, &params, best.data(), nullptr, nullptr), "vgicp_locate_resident");
    std::vector<size_t> order(k);
    for (size_t h = 0; h < k; ++h) {order[h] = h;}
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {return best[a].hits > best[b].hits;});
    const size_t keep = std::min(k, static_cast<size_t>(locate_.keep));
    std::vector<LocateCandidate> found(keep);
    std::vector<Isometry3d> ends(keep);
    for (size_t c = 0; c < keep; ++c) {
      const vgicp_locate_best & b = best[order[c]];
      found[c].poseIndex = static_cast<int>(order[c]);
      found[c].hits = b.hits;
      for (size_t a = 0; a < 3; ++a) {found[c].offset[a] = b.offset[a];}
      found[c].start = shim::poseFromData(b.pose);
      found[c].pose = ends[c] = chainResidentScan(ctx, found[c].start, schedule);
    }
    const std::vector<Evaluation> scores = evaluateResidentScan(ctx, ends);
    size_t winner = 0;
    for (size_t c = 0; c < keep; ++c) {
      found[c].evaluation = scores[c];
      const Evaluation & w = scores[winner];
      if (scores[c].correspondences > w.correspondences ||
        (scores[c].correspondences == w.correspondences && scores[c].cost < w.cost))
      {
        winner = c;
      }
    }
    lastLocation_ = found;
    lastLocationWinner_ = winner;
    lastEvaluation_ = scores[winner];
    return found[winner].pose;
  }
  const std::vector<LocateCandidate> & lastLocation() const {return lastLocation_;}     // of the last locate(), in rank order
  size_t lastLocationWinner() const {return lastLocationWinner_;}

  // A cloud at a pose, point by point (one call of vgicp_points_resident).
  struct PointReport
  {
    uint64_t points = 0;       // of the cloud
    uint64_t matched = 0;      // points whose voxel is in the map at the pose: Evaluation::correspondences there
    uint64_t counted = 0;      // points with weight > 0 under this ICP's robust settings: a robust round's count
    uint64_t negative = 0;     // matched, raw d^2 < 0 (an indefinite covariance)
    uint64_t notFinite = 0;    // matched, raw d^2 NaN or infinite
    std::vector<double> quantiles;      // one order statistic of d^2 per requested quantile, NaN when nothing is ranked
    // per point, in the cloud's order; empty when perPoint was false.  A point without a voxel: +infinity, +infinity, 0, 0
    std::vector<double> d2;             // raw e^T W e, so that d2[i] <= g is "a round gated at g counts point i"
    std::vector<double> squaredError;   // |e|^2
    std::vector<double> weight;
    std::vector<uint8_t> status;        // VGICP_POINT_MATCHED | VGICP_POINT_NEGATIVE | VGICP_POINT_NOT_FINITE
  };

  // Reports `cloud` at `pose`: the resident scan when the cloud still is what CloudPreprocessor::process left on the
  // device (as evaluate decides it), else ONE upload of the cloud.  quantiles: each in [0, 1], at most
  // VGICP_POINT_QUANTILES_MAX; order statistics of max(d^2, 0) over the matched points with a finite d^2, never
  // interpolated.  The weights are those of this ICP's robust settings (setRobust), which are put on the context first.
  // Changes neither the map nor what a later align returns.
  PointReport pointReport(
    const PointCloud & cloud, const LocalMap & localMap, const Isometry3d & pose,
    const std::vector<double> & quantiles = {}, bool perPoint = true)
  {
    if (!vgicp_points_resident) {
      throw std::runtime_error("ICP::pointReport: the linked vgicp module has no vgicp_points_resident (libvgicp_hip_points.so)");
    }
    if (quantiles.size() > static_cast<size_t>(VGICP_POINT_QUANTILES_MAX)) {
      throw std::runtime_error("ICP::pointReport: more than VGICP_POINT_QUANTILES_MAX quantiles");
    }
    vgicp_ctx * ctx = localMap.context();
    applyRobust(ctx);
    lastUsedResidentScan_ = residentScanOrUpload(ctx, cloud, "pointReport");
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    PointReport out;
    vgicp_point_summary summary{};
    const double * q = quantiles.empty() ? nullptr : quantiles.data();
    if (perPoint) {
      // arrays of the host cloud's size; the resident scan says when it is larger (a deferred host copy has not
      // delivered the prepared cloud yet: rule 10 of the header sets summary.points) and the call is made once more
      size_t n = cloud.points_.size();
      for (int attempt = 0;; ++attempt) {
        out.d2.resize(n);
        out.squaredError.resize(n);
        out.weight.resize(n);
        out.status.resize(n);
        summary.points = 0;
        const int rc = vgicp_points_resident(
          ctx, shim::poseData(pose), n, n ? out.d2.data() : nullptr, n ? out.squaredError.data() : nullptr,
          n ? out.weight.data() : nullptr, n ? out.status.data() : nullptr, quantiles.size(), q, &summary, nullptr);
        if (attempt == 0 && static_cast<size_t>(summary.points) > n && (rc == VGICP_ERR_BAD_ARGUMENT || n == 0)) {
          n = static_cast<size_t>(summary.points);
          continue;
        }
        shim::check(ctx, rc, "vgicp_points_resident");
        break;
      }
      n = static_cast<size_t>(summary.points);
      out.d2.resize(n);
      out.squaredError.resize(n);
      out.weight.resize(n);
      out.status.resize(n);
    } else {
      shim::check(
        ctx, vgicp_points_resident(ctx, shim::poseData(pose), 0, nullptr, nullptr, nullptr, nullptr, quantiles.size(), q,
        &summary, nullptr), "vgicp_points_resident");
    }
    out.points = summary.points;
    out.matched = summary.matched;
    out.counted = summary.counted;
    out.negative = summary.negative;
    out.notFinite = summary.not_finite;
    out.quantiles.assign(summary.quantile, summary.quantile + quantiles.size());
    return out;
  }

  // A robust scale c from a quantile of d^2 (PointReport::quantiles): factor * sqrt(d2Quantile).  c is compared with d
  // (c^2 with d^2), so the points below that quantile keep full weight under Huber when factor is 1.  A NaN or
  // non-positive quantile or factor (nothing ranked, or every ranked d^2 zero) is refused.
  static double robustScaleFromQuantile(double d2Quantile, double factor = 1.0)
  {
    if (!(d2Quantile > 0.0) || !(factor > 0.0) || !std::isfinite(d2Quantile) || !std::isfinite(factor)) {
      throw std::invalid_argument("ICP::robustScaleFromQuantile: the quantile of d^2 and the factor must be positive and finite");
    }
    return factor * std::sqrt(d2Quantile);
  }

  // Which hypothesis of a fan to keep, by the score of its RETURNED pose: a converged one goes before one that is not;
  // among equals the lowest Evaluation::score(missPenalty) wins, ties go to the lower index.  hypotheses must not be
  // empty; evaluations[h] scores hypotheses[h].pose.
  static size_t selectBestByScore(
    const std::vector<Hypothesis> & hypotheses, const std::vector<Evaluation> & evaluations,
    double missPenalty = 11.345)
  {
    if (hypotheses.size() != evaluations.size()) {
      throw std::runtime_error("ICP::selectBestByScore: one evaluation per hypothesis");
    }
    size_t best = 0;
    for (size_t h = 1; h < hypotheses.size(); ++h) {
      const bool a = hypotheses[h].converged, b = hypotheses[best].converged;
      if ((a && !b) || (a == b && evaluations[h].score(missPenalty) < evaluations[best].score(missPenalty))) {
        best = h;
      }
    }
    return best;
  }

  // alignHypotheses, evaluate of the returned poses, then the pose of selectBestByScore's choice.  lastStats(),
  // lastBestHypothesis() and lastEvaluation() describe that hypothesis.
  Isometry3d alignBestByScore(
    const PointCloud & cloud, const LocalMap & localMap, const std::vector<Isometry3d> & guesses)
  {
    if (guesses.empty()) {throw std::runtime_error("ICP::alignBestByScore: no guess");}
    const std::vector<Hypothesis> all = alignHypotheses(cloud, localMap, guesses);
    std::vector<Isometry3d> returned;
    returned.reserve(all.size());
    for (const Hypothesis & h : all) {returned.push_back(h.pose);}
    // the fan left the cloud resident (its own upload, or the preparation's): no second upload for the scores
    const std::vector<Evaluation> scores = evaluateResidentScan(localMap.context(), returned);
    const size_t best = selectBestByScore(all, scores);
    lastBest_ = best;
    lastEvaluation_ = scores[best];
    lastStats_.iterations = all[best].iterations;
    lastStats_.converged = all[best].converged;
    lastStats_.seconds = fanSeconds_;
    lastStats_.deviceSeconds = fanDeviceSeconds_;
    lastStats_.correspondenceCounts.assign(
      fanCounts_.begin() + static_cast<std::ptrdiff_t>(best * fanRounds_),
      fanCounts_.begin() + static_cast<std::ptrdiff_t>(best * fanRounds_ + static_cast<size_t>(all[best].iterations)));
    if (!lastStats_.converged) {
      std::cout << "ICP not converged!\n";
    }
    return all[best].pose;
  }

  const Stats & lastStats() const {return lastStats_;}
  const Evaluation & lastEvaluation() const {return lastEvaluation_;}     // of the last alignBestByScore()
  size_t lastBestHypothesis() const {return lastBest_;}                   // of the last alignBest()
  int lastHypothesesPerLaunch() const {return lastHypothesesPerLaunch_;}  // of the last alignHypotheses(): 1 = one by one
  // whether the last align() found its cloud resident on the device (prepared there by CloudPreprocessor::process)
  bool lastUsedResidentScan() const {return lastUsedResidentScan_;}

private:
  ICP() = delete;

  vgicp_params paramsOf() const
  {
    vgicp_params params{};
    params.max_iteration = maxIteration_;
    params.chunk_iterations = chunkIterations_;
    params.translation_sq_threshold = translationSquaredThreshold_;
    params.cosine_threshold = cosineThreshold_;
    return params;
  }

  static void checkSchedule(const std::vector<int> & levels)
  {
    if (levels.size() > static_cast<size_t>(VGICP_LEVEL_STAGES_MAX)) {
      throw std::invalid_argument("ICP: a coarse-to-fine schedule has at most VGICP_LEVEL_STAGES_MAX stages");
    }
    for (const int l : levels) {
      if (l < 0 || l > VGICP_LEVELS_MAX) {
        throw std::invalid_argument("ICP: every level of a coarse-to-fine schedule must be 0 .. VGICP_LEVELS_MAX");
      }
    }
  }

  // the size of a cloud that is about to go up as it is: one covariance per point, or `method` throws
  static size_t pointsWithCovariances(const PointCloud & cloud, const char * method)
  {
    const size_t n = cloud.points_.size();
    if (cloud.covariances_.size() != n) {
      throw std::runtime_error(
              std::string("ICP::") + method + ": the cloud has " + std::to_string(n) + " points but " +
              std::to_string(cloud.covariances_.size()) + " covariances (a cloud prepared with a deferred host "
              "copy and changed since? call shim::materialize first)");
    }
    return n;
  }

  // Use the resident scan or upload this cloud: true when the cloud still is what CloudPreprocessor::process left on the
  // device (the stamp and the hash of the host data say so), else ONE upload of the cloud, which is resident from then on.
  // (align() does not come here: vgicp_align uploads for it, and it may register beside the hash.)
  static bool residentScanOrUpload(vgicp_ctx * ctx, const PointCloud & cloud, const char * method)
  {
    {
      shim::TraceScope ts(shim::Trace::AlignVerify);
      if (shim::residentStampOf(ctx, cloud)) {return true;}
    }
    shim::TraceScope tsCall(shim::Trace::AlignCall);
    const size_t n = pointsWithCovariances(cloud, method);
    const double * pts = n ? cloud.points_.data()->data() : nullptr;
    const double * covs = n ? cloud.covariances_.data()->data() : nullptr;
    shim::check(ctx, vgicp_scan_upload(ctx, n, pts, covs), "vgicp_scan_upload");
    return false;
  }

  // The context may serve several ICP objects: THIS one's robust settings are put on it before each of its aligns.  With
  // the mode off a refusal is not an error (a multi-device context refuses the options and never has the mode on; a
  // stand-in of the C ABI may lack vgicp_set_option, which LocalMap.hpp references weakly); with it on, it is.
  void applyRobust(vgicp_ctx * ctx) const
  {
    const bool on = robustKernel_ != VGICP_ROBUST_NONE || robustGateMicro_ != 0;
    if (!vgicp_set_option) {
      if (on) {throw std::runtime_error("ICP::setRobust: the linked vgicp module has no vgicp_set_option");}
      return;
    }
    const int rcKernel = vgicp_set_option(ctx, VGICP_OPTION_ROBUST_KERNEL, robustKernel_);
    const int rcScale = vgicp_set_option(ctx, VGICP_OPTION_ROBUST_SCALE_MICRO, robustScaleMicro_);
    const int rcGate = vgicp_set_option(ctx, VGICP_OPTION_GATE_MICRO, robustGateMicro_);
    if (on) {
      shim::check(ctx, rcKernel, "vgicp_set_option(VGICP_OPTION_ROBUST_KERNEL)");
      shim::check(ctx, rcScale, "vgicp_set_option(VGICP_OPTION_ROBUST_SCALE_MICRO)");
      shim::check(ctx, rcGate, "vgicp_set_option(VGICP_OPTION_GATE_MICRO)");
    }
  }

  // ... and THIS one's prior, set or cleared.  Without one a refusal is not an error (a multi-device context refuses the
  // call and never has a prior; a stand-in of the C ABI may lack the entry point); with one, it is.
  void applyPrior(vgicp_ctx * ctx) const
  {
    if (!vgicp_set_pose_prior) {
      if (priorOn_) {throw std::runtime_error("ICP::setPrior: the linked vgicp module has no vgicp_set_pose_prior");}
      return;
    }
    if (!priorOn_) {
      (void)vgicp_set_pose_prior(ctx, nullptr, nullptr);
      return;
    }
    shim::check(ctx, vgicp_set_pose_prior(ctx, priorPose_.data(), priorInformation_.data()), "vgicp_set_pose_prior");
  }

  // out = in^-1 for a column-major 6 x 6, Gauss-Jordan with partial pivoting; false for a singular matrix
  static bool invert6(const double * in, double * out)
  {
    double a[6][12];
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) {
        a[r][c] = in[r + 6 * c];
        a[r][6 + c] = r == c ? 1.0 : 0.0;
      }
    }
    for (int k = 0; k < 6; ++k) {
      int p = k;
      for (int r = k + 1; r < 6; ++r) {
        if (std::fabs(a[r][k]) > std::fabs(a[p][k])) {p = r;}
      }
      if (!(std::fabs(a[p][k]) > 0.0)) {return false;}
      for (int c = 0; c < 12; ++c) {std::swap(a[k][c], a[p][c]);}
      const double inv = 1.0 / a[k][k];
      for (int c = 0; c < 12; ++c) {a[k][c] *= inv;}
      for (int r = 0; r < 6; ++r) {
        if (r == k) {continue;}
        const double f = a[r][k];
        for (int c = 0; c < 12; ++c) {a[r][c] -= f * a[k][c];}
      }
    }
    for (int r = 0; r < 6; ++r) {
      for (int c = 0; c < 6; ++c) {out[r + 6 * c] = a[r][6 + c];}
    }
    return true;
  }

  // vgicp_align_resident_levels on whatever scan is resident, over a checked, non-empty schedule: the stages' parameters,
  // the call, the per-stage report (alignCoarseToFine, and locate once per candidate)
  Isometry3d chainResidentScan(vgicp_ctx * ctx, const Isometry3d & guess, const std::vector<int> & schedule)
  {
    const size_t stages = schedule.size();
    std::vector<int32_t> levels(schedule.begin(), schedule.end());
    std::vector<vgicp_params> params(stages, paramsOf());
    for (size_t i = 0; i + 1 < stages; ++i) {
      params[i].max_iteration = coarseMaxIteration_;
      params[i].translation_sq_threshold = coarseTranslationSquaredThreshold_;
      params[i].cosine_threshold = coarseCosineThreshold_;
    }
    std::vector<std::vector<uint64_t>> counts(stages);
    std::vector<vgicp_stats> stats(stages);
    for (size_t i = 0; i < stages; ++i) {
      counts[i].assign(static_cast<size_t>(params[i].max_iteration > 0 ? params[i].max_iteration : 1), 0);
      stats[i] = vgicp_stats{};
      stats[i].corr_count = counts[i].data();
    }
    double pose[16];
    const int rc = vgicp_align_resident_levels(
      ctx, shim::poseData(guess), stages, levels.data(), params.data(), pose, stats.data());
    shim::check(ctx, rc, "vgicp_align_resident_levels");
    lastStages_.assign(stages, StageStats{});
    for (size_t i = 0; i < stages; ++i) {
      StageStats & s = lastStages_[i];
      s.level = schedule[i];
      s.stats.iterations = stats[i].iterations;
      s.stats.converged = stats[i].converged != 0;
      s.stats.seconds = stats[i].seconds;
      s.stats.deviceSeconds = stats[i].device_seconds;
      counts[i].resize(static_cast<size_t>(stats[i].iterations));
      s.stats.correspondenceCounts = counts[i];
    }
    lastStats_ = lastStages_.back().stats;
    if (!lastStats_.converged) {
      std::cout << "ICP not converged!\n";
    }
    return shim::poseFromData(pose);
  }

  // vgicp_evaluate_resident on whatever scan is resident (1 <= poses.size() <= VGICP_EVAL_MAX)
  static std::vector<Evaluation> evaluateResidentScan(vgicp_ctx * ctx, const std::vector<Isometry3d> & poses)
  {
    const size_t k = poses.size();
    std::vector<Evaluation> out;
    std::vector<double> in(16 * k);
    for (size_t h = 0; h < k; ++h) {
      const double * g = shim::poseData(poses[h]);
      for (int e = 0; e < 16; ++e) {in[16 * h + e] = g[e];}
    }
    std::vector<vgicp_evaluation> ev(k);
    shim::check(ctx, vgicp_evaluate_resident(ctx, k, in.data(), ev.data(), nullptr), "vgicp_evaluate_resident");
    out.resize(k);
    for (size_t h = 0; h < k; ++h) {
      out[h].points = ev[h].points;
      out[h].correspondences = ev[h].correspondences;
      out[h].cost = ev[h].cost;
      out[h].squaredError = ev[h].sq_error;
      for (size_t e = 0; e < 27; ++e) {out[h].normalEquations[e] = ev[h].normal_eq[e];}
    }
    return out;
  }

  int maxIteration_;
  double translationSquaredThreshold_;
  double cosineThreshold_;
  int chunkIterations_ = 0;
  int robustKernel_ = VGICP_ROBUST_NONE;
  int robustScaleMicro_ = 1000000;
  int robustGateMicro_ = 0;
  std::vector<int> schedule_;          // of alignCoarseToFine(cloud, map, guess); empty: none
  int coarseMaxIteration_ = 30;
  double coarseTranslationSquaredThreshold_ = 1.0e-4;
  double coarseCosineThreshold_ = 0.999;
  std::vector<StageStats> lastStages_;
  LocalMap::SubmapStats lastSubmap_;
  static constexpr int kLocateKeepMax = 8;
  LocateOptions locate_;               // of locate(cloud, map, guess)
  std::vector<LocateCandidate> lastLocation_;
  size_t lastLocationWinner_ = 0;
  bool priorOn_ = false;
  std::array<double, 16> priorPose_{};
  std::array<double, 36> priorInformation_{};
  Matrix6d posterior_ = Matrix6d::Zero();
  Stats lastStats_;
  bool lastUsedResidentScan_ = false;
  std::vector<uint64_t> fanCounts_;   // the last fan's per-round counts, hypothesis-major
  size_t fanRounds_ = 0;
  double fanSeconds_ = 0.0, fanDeviceSeconds_ = 0.0;
  size_t lastBest_ = 0;
  int lastHypothesesPerLaunch_ = 0;
  Evaluation lastEvaluation_;
};

}  // namespace ESKF_LIO

#endif  // ESKF_LIO_SHIM_REGISTRATION_HPP_
