// LocalMap.hpp — drop-in for the reference's include/ESKF_LIO/LocalMap.hpp + src/LocalMap.cpp.
//
// Same class name, namespace and public methods as the reference (include/ESKF_LIO/LocalMap.hpp:
// 28-61 constructors, :91-98 methods), so src/Odometry.cpp:61,86 and src/ErrorStateKF.cpp:115-130
// compile against it unchanged.  What differs is where the data lives:
//   * the host std::unordered_map stays authoritative (save() and the running-mean insertion rule of
//     Voxel::addPoint, LocalMap.hpp:79-87, need it) and is updated exactly as
//     LocalMap::updateLocalMap does (src/LocalMap.cpp:10-76);
//   * every voxel touched by an update is forwarded to the device mirror as ONE vgicp_map_upsert
//     batch, every evicted voxel as ONE vgicp_map_erase batch, so the HIP registration path reads a
//     table that is current before the next ICP::align;
//   * correspondenceMatching() (src/LocalMap.cpp:78-112) runs on the device through vgicp_match and
//     returns the reference's tuple (srcPoints, srcCovs, mapPoints, mapCovs) in ascending point order
//     (the reference's order is thread-arrival order, i.e. unspecified).
// Deviations, both documented in DESIGN.md: prevTransform_ is initialised (the reference reads it
// uninitialised on the first frame, LocalMap.hpp:113 / LocalMap.cpp:39,134) so the first update
// always inserts; Open3D GUI calls are dropped (visualizeLocalMap() returns true without a window).
// There is no CPU fallback: every method that needs the device throws std::runtime_error with the
// library's message when the HIP module reports an error.
#ifndef ESKF_LIO_SHIM_LOCAL_MAP_HPP_
#define ESKF_LIO_SHIM_LOCAL_MAP_HPP_

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "../vgicp_hip.h"
#include "../vgicp_hip_map_points.h"
#include "../vgicp_hip_map_gated.h"
#include "../vgicp_hip_map_carve.h"
#include "../vgicp_hip_map_rays.h"
#include "../vgicp_hip_map_levels.h"
#include "../vgicp_hip_map_submap.h"
#include "../vgicp_hip_map_checkpoint.h"
#include "../vgicp_hip_map_merge.h"

// The raw-point store's entry points (vgicp_hip_map_points.h, and vgicp_set_option for its option) are referenced
// weakly, so a program that links a stand-in of the C ABI without them (tests/native/shadow_stress.cpp) still links: a
// map then skips switching the option, and one that asks for raw points on the device refuses to be built.  Against the
// module they resolve as usual.  This weakens vgicp_set_option for every translation unit that includes this header
// (INTEGRATION.md §A).
#pragma weak vgicp_map_points_size
#pragma weak vgicp_map_points_export
#pragma weak vgicp_set_option
// ... and so are the gated insertion's (vgicp_hip_map_gated.h, in libvgicp_hip_map_gated.so beside the module): a program
// that links without that library builds maps as before, and setInsertGate(g > 0) refuses.
#pragma weak vgicp_map_insert_resident_gated_async
#pragma weak vgicp_map_gated_totals
// ... and free-space carving's (vgicp_hip_map_carve.h, in libvgicp_hip_map_carve.so): without that library setCarve refuses.
#pragma weak vgicp_map_carve_resident_async
#pragma weak vgicp_map_carve_totals
// ... and the ray report's (vgicp_hip_map_rays.h, in libvgicp_hip_map_rays.so): without that library rayReport and rayCounts
// say available == false.
#pragma weak vgicp_rays_resident
// ... and the map levels' (vgicp_hip_map_levels.h, in libvgicp_hip_map_levels.so): without that library setLevels(n > 0) refuses.
#pragma weak vgicp_map_levels_build
// ... and the submap's (vgicp_hip_map_submap.h, in libvgicp_hip_map_submap.so): without that library scanFromMap refuses.
#pragma weak vgicp_scan_from_map
#pragma weak vgicp_scan_from_map_keys
// ... and the map checkpoint's (vgicp_hip_map_checkpoint.h, in libvgicp_hip_map_checkpoint.so): without that library
// saveCheckpoint and loadCheckpoint refuse.
#pragma weak vgicp_map_checkpoint_size
#pragma weak vgicp_map_checkpoint
#pragma weak vgicp_map_restore
// ... and the map merge's (vgicp_hip_map_merge.h, in libvgicp_hip_map_merge.so): without that library mergeFrom refuses.
#pragma weak vgicp_map_merge
#include "ShimTypes.hpp"
#include "ShimSupport.hpp"
#include "ResidentScan.hpp"
#include "UpdatePlan.hpp"

#if defined(ESKF_LIO_SHIM_NATIVE_TYPES) && __has_include(<yaml-cpp/yaml.h>)
#include <yaml-cpp/yaml.h>
#define ESKF_LIO_SHIM_HAVE_YAML 1
#endif

namespace ESKF_LIO
{

// The keys LocalMap's YAML constructor reads (config/hilti_config.yaml:36-45).
struct LocalMapConfig
{
  double voxelSize = 0.3;
  size_t maxNumPointsPerVoxel = 1000;
  double translationSquaredThreshold = 1.0e-2;
  double cosineThreshold = 0.985;
  bool removeDistantPoints = true;
  double distanceThreshold = 100.0;
  double removePeriod = 10.0;
  // false: the host std::unordered_map is authoritative and the device mirror is fed batches (keeps
  //        every raw point for save(), as the reference does).
  // true:  the voxel grid the registration reads lives on the device — insertion and eviction run there
  //        (vgicp_map_insert_resident_async / vgicp_map_evict, same arithmetic, same results, nothing waited for).
  //        With keepRawPoints the raw points every voxel holds (what save() writes, src/LocalMap.cpp:156-167) are kept
  //        in a host-side SHADOW of the grid that a worker thread of this object maintains from the prepared clouds
  //        updateLocalMap is handed (the reference's own insertion and eviction loops, in the reference's order, off
  //        the caller's thread): save() then writes exactly what the reference writes.  The shadow needs the prepared
  //        scan on the host (CloudPreprocessorConfig::HostCopy::Eager, the default); with a deferred host copy, or
  //        with keepRawPoints = false, save() writes one point per voxel (its mean).
  // Default since round 5: true / true — the classes as a maintainer gets them by swapping the headers are the fast
  // ones (0.5 - 0.6 ms per 60 000-point frame instead of 3.6 - 4.5), and save() still writes the reference's content.
  bool deviceResident = true;
  bool keepRawPoints = true;
  // With deviceResident and keepRawPoints: the raw points are kept by the device map itself
  // (VGICP_OPTION_MAP_RAW_POINTS, include/vgicp_hip_map_points.h; 32 bytes per kept point on the device) instead of the
  // shadow grid — no worker thread, no host copy of the prepared scan needed, and save() writes every raw point
  // whatever the host-copy mode.  YAML: local_map.raw_points_on_device (optional, default false).
  bool rawPointsOnDevice = false;
  // > 0 (or +infinity): updateLocalMap keeps the points out of the map that are matched at the frame's pose and fail
  // max(d^2, 0) <= insertGate (LocalMap::setInsertGate; include/vgicp_hip_map_gated.h has the rule and the units, which
  // are ICP::robustScaleFromQuantile's).  0: off.  YAML: local_map.insert_gate (optional, default 0).
  double insertGate = 0.0;
  // carve: every updateLocalMap whose cloud is still the resident scan first removes the voxels that scan sees through
  // (LocalMap::setCarve; include/vgicp_hip_map_carve.h has the rule).  YAML: local_map.carve.{margin, max_range,
  // min_hits, stride, origin} (optional; carving is off unless local_map.carve is there, and max_range is required then).
  bool carve = false;
  vgicp_carve_params carveParams = {{0.0, 0.0, 0.0}, 0.0, 0.0, 1, 1};
  // > 0: the device keeps the map again at 2, 4, .. 2^levels times the voxel size (LocalMap::setLevels;
  // include/vgicp_hip_map_levels.h has the rule), for ICP::alignCoarseToFine.  YAML: the largest level of
  // registration.coarse_to_fine.levels (optional; no levels unless it is there).
  int levels = 0;
};

class LocalMap
{
public:
  struct Voxel;

  using PointVector = typename std::vector<Vector3d>;
  using CovarianceVector = typename std::vector<Matrix3d>;
  using Correspondence = typename std::tuple<PointVector, CovarianceVector, PointVector,
      CovarianceVector>;

  struct Key
  {
    int32_t i, j, k;
    bool operator==(const Key & o) const {return i == o.i && j == o.j && k == o.k;}
  };
  // open3d::utility::hash_eigen<Eigen::Vector3i> (boost-style combine); only iteration order
  // depends on it.
  struct VoxelHash
  {
    size_t operator()(const Key & key) const
    {
      size_t seed = 0;
      const int32_t e[3] = {key.i, key.j, key.k};
      for (int n = 0; n < 3; ++n) {
        seed ^= std::hash<int>()(e[n]) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
      }
      return seed;
    }
  };
  using VoxelGrid = typename std::unordered_map<Key, Voxel, VoxelHash>;

  struct Voxel
  {
    size_t maxNumPoints;
    size_t numPoints;
    PointVector points;
    Vector3d mean;
    Matrix3d covariance;
    bool dirty = false;  // touched since the last device sync

    Voxel(size_t maxNumPoints_, const Vector3d & point, const Matrix3d & covariance_)
    : maxNumPoints(maxNumPoints_), numPoints(1), mean(point), covariance(covariance_)
    {
      points.reserve(maxNumPoints);
      points.push_back(point);
    }

    // returns true when the voxel changed
    bool addPoint(const Vector3d & point, const Matrix3d & covariance_)
    {
      if (numPoints >= maxNumPoints) {return false;}
      points.push_back(point);
      const double n = static_cast<double>(numPoints), n1 = static_cast<double>(numPoints + 1);
      for (int a = 0; a < 3; ++a) {mean(a) = (n * mean(a) + point(a)) / n1;}
      for (int c = 0; c < 3; ++c) {
        for (int r = 0; r < 3; ++r) {
          covariance(r, c) = (n * covariance(r, c) + covariance_(r, c)) / n1;
        }
      }
      ++numPoints;
      return true;
    }
  };

  explicit LocalMap(const LocalMapConfig & config, bool visualize = false, vgicp_ctx * ctx = nullptr)
  : voxelSize_(config.voxelSize)
    , maxNumPointsPerVoxel_(config.maxNumPointsPerVoxel)
    , translationSquaredThreshold_(config.translationSquaredThreshold)
    , cosineThreshold_(config.cosineThreshold)
    , removeDistantPoints_(config.removeDistantPoints)
    , distanceThreshold_(config.distanceThreshold)
    , removePeriod_(config.removePeriod)
    , deviceResident_(config.deviceResident)
    , keepRawPoints_(config.keepRawPoints)
    , rawOnDevice_(config.deviceResident && config.keepRawPoints && config.rawPointsOnDevice)
    , visualize_(visualize)
    , ctx_(ctx ? ctx : shim::defaultContext())
  {
    shim::check(ctx_, vgicp_map_reset(ctx_, voxelSize_, 0), "vgicp_map_reset");
    storeRawPointsOnDevice();
    if (config.insertGate != 0.0) {setInsertGate(config.insertGate);}
    if (config.carve) {setCarve(config.carveParams);}
    if (config.levels != 0) {setLevels(config.levels);}
  }

  ~LocalMap() {shadowStop();}
  LocalMap(const LocalMap &) = delete;
  LocalMap & operator=(const LocalMap &) = delete;

  // reference: LocalMap(double voxelSize, size_t maxNumPointsPerVoxel, bool visualize = false).
  // The reference leaves the update thresholds uninitialised here (LocalMap.hpp:54-61); this one
  // disables the motion gate and the eviction instead, i.e. every update inserts.
  LocalMap(double voxelSize, size_t maxNumPointsPerVoxel, bool visualize = false,
    vgicp_ctx * ctx = nullptr)
  : voxelSize_(voxelSize)
    , maxNumPointsPerVoxel_(maxNumPointsPerVoxel)
    , translationSquaredThreshold_(-1.0)
    , cosineThreshold_(2.0)
    , removeDistantPoints_(false)
    , distanceThreshold_(std::numeric_limits<double>::infinity())
    , removePeriod_(std::numeric_limits<double>::infinity())
    , visualize_(visualize)
    , ctx_(ctx ? ctx : shim::defaultContext())
  {
    shim::check(ctx_, vgicp_map_reset(ctx_, voxelSize_, 0), "vgicp_map_reset");
    storeRawPointsOnDevice();
  }

#if defined(ESKF_LIO_SHIM_HAVE_YAML)
  // reference: LocalMap(const YAML::Node &, const PinholeCameraParameters &, bool visualize = true)
  LocalMap(
    const YAML::Node & config, const open3d::camera::PinholeCameraParameters &,
    bool visualize = true)
  : LocalMap(fromYaml(config), visualize) {}

  static LocalMapConfig fromYaml(const YAML::Node & config)
  {
    LocalMapConfig c;
    const auto & m = config["local_map"];
    c.voxelSize = m["voxel_size"].as<double>();
    c.maxNumPointsPerVoxel = m["max_num_points_per_voxel"].as<size_t>();
    c.translationSquaredThreshold = m["update"]["translation_sq_threshold"].as<double>();
    c.cosineThreshold = m["update"]["cosine_threshold"].as<double>();
    c.removeDistantPoints = m["remove_distant_points"]["enabled"].as<bool>();
    c.distanceThreshold = m["remove_distant_points"]["distance_threshold"].as<double>();
    c.removePeriod = m["remove_distant_points"]["removing_period"].as<double>();
    if (m["raw_points_on_device"].IsDefined()) {c.rawPointsOnDevice = m["raw_points_on_device"].as<bool>();}
    if (m["insert_gate"].IsDefined()) {c.insertGate = m["insert_gate"].as<double>();}
    if (m["carve"].IsDefined()) {
      const auto & k = m["carve"];
      c.carve = true;
      c.carveParams.max_range = k["max_range"].as<double>();
      if (k["margin"].IsDefined()) {c.carveParams.margin = k["margin"].as<double>();}
      if (k["min_hits"].IsDefined()) {c.carveParams.min_hits = k["min_hits"].as<uint32_t>();}
      if (k["stride"].IsDefined()) {c.carveParams.stride = k["stride"].as<uint32_t>();}
      if (k["origin"].IsDefined()) {
        const std::vector<double> origin = k["origin"].as<std::vector<double>>();
        if (origin.size() != 3) {throw std::invalid_argument("local_map.carve.origin: three numbers");}
        for (int a = 0; a < 3; ++a) {c.carveParams.origin[a] = origin[a];}
      }
    }
    // the schedule is the registration's (ICP reads it); the map keeps the levels it names
    if (config["registration"].IsDefined() && config["registration"]["coarse_to_fine"].IsDefined() &&
      config["registration"]["coarse_to_fine"]["levels"].IsDefined())
    {
      for (const int l : config["registration"]["coarse_to_fine"]["levels"].as<std::vector<int>>()) {
        if (l < 0 || l > VGICP_LEVELS_MAX) {
          throw std::invalid_argument("registration.coarse_to_fine.levels: each 0 .. VGICP_LEVELS_MAX");
        }
        c.levels = std::max(c.levels, l);
      }
    }
    return c;
  }
#endif

  // reference: src/LocalMap.cpp:10-76. The cloud is moved into the world frame in place, as there.  What this update does
  // is decided once (UpdatePlan.hpp; DESIGN.md §9 has the table); the rest carries it out.
  void updateLocalMap(PointCloudPtr cloud, const Isometry3d & transform, bool initialize = false)
  {
    using Plan = shim::UpdatePlan;
    // a cloud that ends its life here (moved in by its only owner, src/Odometry.cpp:86, and not passed on to the shadow
    // grid's worker) leaves its buffers to the frames to come
    struct Recycler
    {
      PointCloudPtr & c;
      ~Recycler() {if (c && c.use_count() == 1) {shim::recycleStorage(*c);}}
    } recycler{cloud};
    // The cloud CloudPreprocessor::process prepared and ICP::align registered is still resident on the device
    // (src/Odometry.cpp:74,79,86 pass the same cloud along): with the grid on the device the insertion runs there
    // on that resident scan, enqueued only — no upload, nothing waited for.
    shim::UpdateFacts facts;
    {
      shim::TraceScope ts(shim::Trace::UpdateVerify);
      const shim::ResidentStamp * stamp = deviceResident_ ? shim::residentStampOf(ctx_, *cloud) : nullptr;
      facts.resident = stamp != nullptr;
      facts.hostIsCurrent = stamp && stamp->hostIsCurrent;
    }
    shim::TraceScope tsRest(shim::Trace::UpdateRest);
    facts.deviceResident = deviceResident_;
    facts.keepRawPoints = keepRawPoints_;
    facts.rawOnDevice = rawOnDevice_;
    facts.shadowComplete = shadowComplete_;
    facts.initialize = initialize;
    facts.hasPrevTransform = hasPrevTransform_;
    facts.moved = !initialize && hasPrevTransform_ && needsMapUpdate(transform);
    facts.evictionDue = shim::insertionDue(facts) && removeDistantPoints_ && now() - currentRemoveTime_ > removePeriod_;
    facts.soleOwner = cloud.use_count() == 1;
    facts.gated = insertGate_ > 0.0;
    facts.carve = carve_;
    const Plan plan = shim::planUpdate(facts);

    if (plan.route != Plan::Route::ResidentScan) {
      shim::materialize(ctx_, *cloud);   // a cloud whose prepared scan is on the device only: the host map needs the data
      cloud->Transform(transform.matrix());
    }
    trajectory_.push_back(transform);
    if (plan.insert) {
      const Vector3d position = transform.translation();
      if (plan.route == Plan::Route::HostMap) {
        updateHostMap(*cloud, position, plan.evict);
      } else {
        if (plan.route == Plan::Route::ResidentScan) {
          shim::TraceScope tsInsert(shim::Trace::UpdateInsert);
          if (plan.carve) {
            shim::check(
              ctx_, vgicp_map_carve_resident_async(ctx_, shim::poseData(transform), &carveParams_),
              "vgicp_map_carve_resident_async");
          }
          if (plan.entry == Plan::Entry::Gated) {
            shim::check(
              ctx_, vgicp_map_insert_resident_gated_async(
                ctx_, shim::poseData(transform), maxNumPointsPerVoxel_, insertGate_),
              "vgicp_map_insert_resident_gated_async");
          } else {
            shim::check(
              ctx_, vgicp_map_insert_resident_async(ctx_, shim::poseData(transform), maxNumPointsPerVoxel_),
              "vgicp_map_insert_resident_async");
          }
        } else if (!cloud->points_.empty()) {
          // the cloud is already in the world frame (transformed in place above, as the reference does)
          const Isometry3d identity = Isometry3d::Identity();
          shim::check(
            ctx_, vgicp_map_insert_scan(
              ctx_, cloud->points_.size(), cloud->points_.data()->data(), cloud->covariances_.data()->data(),
              shim::poseData(identity), maxNumPointsPerVoxel_, nullptr), "vgicp_map_insert_scan");
        }
        if (plan.countPlain) {++plainFrames_;}
        if (plan.evict) {evictOnDevice(position);}
      }
      hasPrevTransform_ = true;
    }
    prevTransform_ = transform;
    // the resident route's host side, for save(): in place here (src/LocalMap.cpp:15; the stamp is void now) unless the
    // worker does it, on a cloud nobody else can see
    if (plan.route == Plan::Route::ResidentScan && plan.transform == Plan::Transform::Here) {
      cloud->Transform(transform.matrix());
    }
    if (plan.handOver != Plan::HandOver::None) {shadowHandOver(plan, cloud, transform);}
    shadowComplete_ = plan.shadowComplete;
    if (plan.route == Plan::Route::ResidentScan) {shim::forget(ctx_);}
  }

  // reference: src/LocalMap.cpp:78-112 (device lookup; ascending point order).
  Correspondence correspondenceMatching(
    const PointVector & points, const CovarianceVector & covariances) const
  {
    Correspondence correspondence;
    auto & [srcPoints, srcCovs, mapPoints, mapCovs] = correspondence;
    const size_t n = points.size();
    srcPoints.resize(n);
    srcCovs.resize(n);
    mapPoints.resize(n);
    mapCovs.resize(n);
    size_t matched = 0;
    if (n > 0) {
      shim::check(
        ctx_, vgicp_match(
          ctx_, n, points.data()->data(), covariances.data()->data(),
          srcPoints.data()->data(), srcCovs.data()->data(), mapPoints.data()->data(),
          mapCovs.data()->data(), nullptr, &matched), "vgicp_match");
    }
    srcPoints.resize(matched);
    srcCovs.resize(matched);
    mapPoints.resize(matched);
    mapCovs.resize(matched);
    return correspondence;
  }

  // reference: src/LocalMap.cpp:120-130 polls an Open3D window; there is none here.
  bool visualizeLocalMap() const {return true;}

  // reference: src/LocalMap.cpp:156-167 writes a .pcd through Open3D and a PinholeCameraTrajectory
  // JSON. Written here without Open3D: ASCII PCD v0.7 — of every stored point when the host map is
  // authoritative (as the reference writes) or the raw points are kept (by the device map, read back with
  // vgicp_map_points_export, or by the shadow grid), else of ONE point per voxel (its mean, read back with
  // vgicp_map_export) in deviceResident mode — and the 4x4 poses as a JSON array of column-major
  // "extrinsic" arrays (the field Open3D's trajectory reader uses).
  void save(const std::string & cloud_path, const std::string & trajectory_path) const
  {
    shadowDrain();
    std::vector<double> deviceMeans;   // or the device map's raw points
    if (rawOnDevice_) {
      size_t n = 0, written = 0;
      shim::check(ctx_, vgicp_map_points_size(ctx_, &n, nullptr), "vgicp_map_points_size");
      std::vector<int32_t> keys(3 * n);
      deviceMeans.resize(3 * n);
      if (n) {
        shim::check(
          ctx_, vgicp_map_points_export(ctx_, n, keys.data(), deviceMeans.data(), &written),
          "vgicp_map_points_export");
      }
      deviceMeans.resize(3 * written);
    } else if (deviceResident_ && !(keepRawPoints_ && shadowComplete_)) {
      const size_t n = size();
      std::vector<int32_t> keys(3 * n);
      std::vector<double> covs(9 * n);
      std::vector<uint64_t> counts(n);
      deviceMeans.resize(3 * n);
      size_t written = 0;
      if (n) {
        shim::check(
          ctx_, vgicp_map_export(
            ctx_, n, keys.data(), deviceMeans.data(), covs.data(), counts.data(),
            &written), "vgicp_map_export");
      }
      deviceMeans.resize(3 * written);
    }
    size_t total = deviceMeans.size() / 3;
    for (const auto & kv : voxelGrid_) {total += kv.second.points.size();}
    std::ofstream pcd(cloud_path);
    pcd << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\n"
        << "TYPE F F F\nCOUNT 1 1 1\nWIDTH " << total << "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
        << "POINTS " << total << "\nDATA ascii\n";
    pcd.precision(17);
    for (const auto & kv : voxelGrid_) {
      for (const auto & p : kv.second.points) {pcd << p(0) << ' ' << p(1) << ' ' << p(2) << '\n';}
    }
    for (size_t v = 0; v + 2 < deviceMeans.size(); v += 3) {
      pcd << deviceMeans[v] << ' ' << deviceMeans[v + 1] << ' ' << deviceMeans[v + 2] << '\n';
    }
    std::ofstream traj(trajectory_path);
    traj.precision(17);
    traj << "{\n\"class_name\" : \"PinholeCameraTrajectory\",\n\"parameters\" : [\n";
    for (size_t t = 0; t < trajectory_.size(); ++t) {
      const double * m = shim::poseData(trajectory_[t]);
      traj << "{ \"extrinsic\" : [";
      for (int e = 0; e < 16; ++e) {traj << (e ? ", " : " ") << m[e];}
      traj << " ] }" << (t + 1 < trajectory_.size() ? ",\n" : "\n");
    }
    traj << "],\n\"version_major\" : 1,\n\"version_minor\" : 0\n}\n";
  }

  // ---- additions (not in the reference) ----
  size_t size() const
  {
    if (!deviceResident_) {return voxelGrid_.size();}
    size_t voxels = 0;
    shim::check(ctx_, vgicp_map_size(ctx_, &voxels, nullptr), "vgicp_map_size");
    return voxels;
  }
  bool deviceResident() const {return deviceResident_;}
  double voxelSize() const {return voxelSize_;}
  vgicp_ctx * context() const {return ctx_;}
  // the host's voxel grid: authoritative without deviceResident, else the shadow kept for save() (brought up to date first)
  const VoxelGrid & grid() const
  {
    shadowDrain();
    return voxelGrid_;
  }
  // true while save() will write every stored raw point, as the reference does (false once a frame was inserted on the
  // device whose prepared scan never reached the host)
  bool savesRawPoints() const {return !deviceResident_ || rawOnDevice_ || (keepRawPoints_ && shadowComplete_);}
  // the device map keeps the raw points (LocalMapConfig::rawPointsOnDevice)
  bool rawPointsOnDevice() const {return rawOnDevice_;}

  // Gated insertion (include/vgicp_hip_map_gated.h): from the next updateLocalMap on, a frame whose cloud is still the
  // resident scan is inserted without the points that are matched at its pose and fail max(d^2, 0) <= gate, on the
  // device and enqueued only, as the plain insertion is.  gate: finite and >= 0, or +infinity, in the units of
  // ICP::robustScaleFromQuantile; 0 switches the gate off, and the map then behaves exactly as without this call.
  // A device-resident map only.  A map that keeps raw points for save() must read them from the device from here on
  // (the shadow grid would file the refused points too): the store is switched on, which the module accepts while the map
  // is empty — so set the gate before the first frame, or build the map with rawPointsOnDevice.
  void setInsertGate(double gate)
  {
    if (!(gate >= 0.0)) {
      throw std::invalid_argument("LocalMap::setInsertGate: the gate is finite and >= 0 (0: off), or +infinity");
    }
    if (gate > 0.0) {
      if (!deviceResident_) {
        throw std::invalid_argument("LocalMap::setInsertGate: only a device-resident map inserts the resident scan");
      }
      if (!(vgicp_map_insert_resident_gated_async && vgicp_map_gated_totals)) {
        throw std::runtime_error("LocalMap::setInsertGate: the linked vgicp module has no gated insertion");
      }
      if (keepRawPoints_ && !rawOnDevice_) {
        shadowDrain();
        rawOnDevice_ = true;
        try {
          storeRawPointsOnDevice();
        } catch (...) {
          rawOnDevice_ = false;
          throw;
        }
      }
    }
    insertGate_ = gate;
  }
  double insertGate() const {return insertGate_;}
  struct GatedTotals
  {
    uint64_t points = 0, refused = 0;   // of the gated insertions since the map was made (vgicp_map_gated_totals: settles)
    uint64_t plainFrames = 0;           // frames inserted whole while a gate was set: their cloud was no resident scan
  };
  GatedTotals gatedTotals() const
  {
    GatedTotals t;
    t.plainFrames = plainFrames_;
    if (vgicp_map_gated_totals) {
      shim::check(ctx_, vgicp_map_gated_totals(ctx_, &t.points, &t.refused), "vgicp_map_gated_totals");
    }
    return t;
  }

  // Free-space carving (include/vgicp_hip_map_carve.h): from the next updateLocalMap on, a frame whose cloud is still the
  // resident scan first removes from the map the voxels that at least min_hits of its rays cross and that hold none of
  // its returns — at the frame's pose, on the device, enqueued only — and is inserted then.  params.origin is the
  // sensor's origin in the prepared scan's frame: the translation of the extrinsic the preparation applied.
  // A device-resident map only; its raw points move to the device as for setInsertGate (set it before the first frame).
  void setCarve(const vgicp_carve_params & params)
  {
    const bool finite = std::isfinite(params.origin[0]) && std::isfinite(params.origin[1]) && std::isfinite(params.origin[2]);
    if (!finite || !(params.margin >= 0.0) || std::isinf(params.margin) || !(params.max_range > 0.0) ||
      std::isinf(params.max_range) || !(params.max_range / voxelSize_ <= VGICP_CARVE_MAX_STEPS) || params.min_hits == 0 ||
      params.stride == 0)
    {
      throw std::invalid_argument(
              "LocalMap::setCarve: origin finite, margin finite and >= 0, max_range finite, > 0 and at most "
              "VGICP_CARVE_MAX_STEPS voxel sizes, min_hits and stride >= 1");
    }
    if (!deviceResident_) {
      throw std::invalid_argument("LocalMap::setCarve: only a device-resident map holds the resident scan's rays");
    }
    if (!(vgicp_map_carve_resident_async && vgicp_map_carve_totals)) {
      throw std::runtime_error("LocalMap::setCarve: the linked vgicp module has no free-space carving");
    }
    if (keepRawPoints_ && !rawOnDevice_) {
      shadowDrain();
      rawOnDevice_ = true;
      try {
        storeRawPointsOnDevice();
      } catch (...) {
        rawOnDevice_ = false;
        throw;
      }
    }
    carveParams_ = params;
    carve_ = true;
  }
  void clearCarve() {carve_ = false;}
  bool carving() const {return carve_;}
  struct CarveTotals
  {
    uint64_t rays = 0, removed = 0;   // since the map was made (vgicp_map_carve_totals: settles)
  };
  CarveTotals carveTotals() const
  {
    CarveTotals t;
    if (vgicp_map_carve_totals) {
      shim::check(ctx_, vgicp_map_carve_totals(ctx_, &t.rays, &t.removed), "vgicp_map_carve_totals");
    }
    return t;
  }

  // The map's coarser levels (include/vgicp_hip_map_levels.h): from now on the device keeps the map again at 2, 4, ..
  // 2^levels times its voxel size and brings the levels up to date whenever ICP::alignCoarseToFine reads them after the
  // map has changed (two launches per level, nothing when the map did not change).  0 releases them.  None of the
  // drop-in calls changes its route.
  void setLevels(int levels)
  {
    if (levels < 0 || levels > VGICP_LEVELS_MAX) {
      throw std::invalid_argument("LocalMap::setLevels: levels must be 0 .. VGICP_LEVELS_MAX");
    }
    if (!vgicp_map_levels_build) {
      if (levels == 0) {return;}
      throw std::runtime_error("LocalMap::setLevels: the linked vgicp module has no map levels (libvgicp_hip_map_levels.so)");
    }
    shim::check(ctx_, vgicp_map_levels_build(ctx_, levels, nullptr), "vgicp_map_levels_build");
    levels_ = levels;
  }
  int levels() const {return levels_;}

  // Submap as scan (include/vgicp_hip_map_submap.h): the resident scan of THIS map's context becomes the voxels of
  // `source` (this map itself, or another map on the same device; with level > 0 that level of it, LocalMap::setLevels)
  // whose centres lie within `radius` of `center` (in source's frame; infinity: all of them) and that hold at least
  // minCount points, each moved by `frame` — on the device, in the order of source's table.  Every call over the
  // resident scan then registers, scores or inserts a piece of map (ICP::alignSubmap is the loop-closure recipe).  The
  // cloud CloudPreprocessor::process left on the device is no longer resident afterwards: an align of it uploads it.
  // points == 0: nothing was selected and no scan is resident.  Both maps must keep their voxels on the device.
  struct SubmapStats
  {
    uint64_t voxels = 0, points = 0, tooFar = 0, tooFew = 0;
    double seconds = 0.0, deviceSeconds = 0.0;
  };
  SubmapStats scanFromMap(
    const LocalMap & source, const Vector3d & center, double radius, const Isometry3d & frame, size_t minCount = 0,
    int level = 0)
  {
    if (!vgicp_scan_from_map) {
      throw std::runtime_error("LocalMap::scanFromMap: the linked vgicp module has no vgicp_scan_from_map (libvgicp_hip_map_submap.so)");
    }
    if (!deviceResident_ || !source.deviceResident_) {
      throw std::runtime_error("LocalMap::scanFromMap: both maps must be device-resident");
    }
    vgicp_submap_params p{};
    for (int a = 0; a < 3; ++a) {p.center[a] = center.data()[a];}
    p.radius = radius;
    const double * f = shim::poseData(frame);
    for (int e = 0; e < 16; ++e) {p.frame[e] = f[e];}
    p.min_count = minCount;
    p.level = level;
    vgicp_submap_stats st{};
    shim::check(ctx_, vgicp_scan_from_map(ctx_, source.ctx_, &p, &st), "vgicp_scan_from_map");
    SubmapStats out;
    out.voxels = st.voxels;
    out.points = st.points;
    out.tooFar = st.too_far;
    out.tooFew = st.too_few;
    out.seconds = st.seconds;
    out.deviceSeconds = st.device_seconds;
    return out;
  }
  // The keys (3 per point) and counts of the voxels behind the resident scan scanFromMap made, in scan order.
  void scanFromMapKeys(std::vector<int32_t> & keys, std::vector<uint64_t> & counts) const
  {
    if (!vgicp_scan_from_map_keys) {
      throw std::runtime_error("LocalMap::scanFromMapKeys: the linked vgicp module has no vgicp_scan_from_map_keys (libvgicp_hip_map_submap.so)");
    }
    size_t n = 0;
    const int rc = vgicp_scan_from_map_keys(ctx_, 0, nullptr, nullptr, &n);   // size query
    if (rc != VGICP_OK && !(rc == VGICP_ERR_BAD_ARGUMENT && n > 0)) {shim::check(ctx_, rc, "vgicp_scan_from_map_keys");}
    keys.assign(3 * n, 0);
    counts.assign(n, 0);
    shim::check(ctx_, vgicp_scan_from_map_keys(ctx_, n, keys.data(), counts.data(), &n), "vgicp_scan_from_map_keys");
  }

  // Map merge (include/vgicp_hip_map_merge.h): the voxels of `source` whose centres lie within `radius` of `center` (in
  // source's frame; infinity: all of them) and that hold at least minCount points are moved by `frame` (source's map ->
  // this map: the pose ICP::alignSubmap returned, times the anchor's inverse) and folded into THIS map, each weighted by
  // its count, on the device.  A voxel of this map that holds maxCount points or more accepts nothing (0: no cap).
  // Beside the drop-in calls: none of them changes its route, and the resident scan stays.  Both maps must keep their
  // voxels on the device; where this map's points live in the host's shadow grid (no deviceResident, or keepRawPoints
  // without rawPointsOnDevice) the method throws, as loadCheckpoint does: the shadow grid would not see the merged voxels
  // (with rawPointsOnDevice the module refuses: a merged voxel has no point list to keep).
  struct MergeStats
  {
    uint64_t voxels = 0, selected = 0, tooFar = 0, tooFew = 0, created = 0, updated = 0, frozen = 0, points = 0;
    double seconds = 0.0, deviceSeconds = 0.0;
  };
  MergeStats mergeFrom(
    const LocalMap & source, const Isometry3d & frame, const Vector3d & center, double radius, size_t minCount = 0,
    size_t maxCount = 0)
  {
    if (!vgicp_map_merge) {
      throw std::runtime_error("LocalMap::mergeFrom: the linked vgicp module has no vgicp_map_merge (libvgicp_hip_map_merge.so)");
    }
    if (!deviceResident_ || !source.deviceResident_) {
      throw std::runtime_error("LocalMap::mergeFrom: both maps must be device-resident");
    }
    if (keepRawPoints_ && !rawOnDevice_) {
      throw std::runtime_error(
              "LocalMap::mergeFrom: the map's points live in the host's shadow grid, which a merge does not reach "
              "(deviceResident, and without keepRawPoints)");
    }
    vgicp_merge_params p{};
    for (int a = 0; a < 3; ++a) {p.center[a] = center.data()[a];}
    p.radius = radius;
    const double * f = shim::poseData(frame);
    for (int e = 0; e < 16; ++e) {p.frame[e] = f[e];}
    p.min_count = minCount;
    p.max_count = maxCount;
    vgicp_merge_stats st{};
    shim::check(ctx_, vgicp_map_merge(ctx_, source.ctx_, &p, &st), "vgicp_map_merge");
    MergeStats out;
    out.voxels = st.voxels;
    out.selected = st.selected;
    out.tooFar = st.too_far;
    out.tooFew = st.too_few;
    out.created = st.created;
    out.updated = st.updated;
    out.frozen = st.frozen;
    out.points = st.points;
    out.seconds = st.seconds;
    out.deviceSeconds = st.device_seconds;
    return out;
  }

  // The map checkpoint (include/vgicp_hip_map_checkpoint.h): the device map as one blob, restored slot for slot, so that a
  // stopped session goes on with the bits it would have produced.  The file is the blob verbatim, then a trailer:
  // "VGICPTRJ", u64 n, the n trajectory poses and prevTransform_ as 16 doubles each (column-major).  Written to
  // path + ".tmp" and renamed.  Beside the drop-in calls: none of them changes its route.  Where the map's points live in
  // the host's shadow grid (no deviceResident, or keepRawPoints without rawPointsOnDevice) both methods throw: the shadow
  // grid is not restored.  A file whose raw-points flag or voxel_size is not this map's (voxel_size bit for bit) is
  // refused before anything is loaded.  The trailer does not carry whether prevTransform_ was ever set by an insertion
  // (hasPrevTransform_, which updateLocalMap sets with its first insertion): a load takes it to be set exactly when the
  // trajectory is not empty, which is what it is after every update that inserted — every first update does.
  void saveCheckpoint(const std::string & path)
  {
    requireCheckpoint("saveCheckpoint");
    size_t bytes = 0;
    shim::check(ctx_, vgicp_map_checkpoint_size(ctx_, &bytes), "vgicp_map_checkpoint_size");
    std::vector<char> blob(bytes);
    shim::check(ctx_, vgicp_map_checkpoint(ctx_, blob.size(), blob.data(), &bytes, nullptr), "vgicp_map_checkpoint");
    const std::string tmp = path + ".tmp";
    {
      std::ofstream out(tmp, std::ios::binary | std::ios::trunc);
      out.write(blob.data(), static_cast<std::streamsize>(bytes));
      out.write("VGICPTRJ", 8);
      const uint64_t n = trajectory_.size();
      out.write(reinterpret_cast<const char *>(&n), 8);
      for (const Isometry3d & pose : trajectory_) {out.write(reinterpret_cast<const char *>(shim::poseData(pose)), 128);}
      out.write(reinterpret_cast<const char *>(shim::poseData(prevTransform_)), 128);
      out.flush();
      if (!out) {throw std::runtime_error("LocalMap::saveCheckpoint: cannot write " + tmp);}
    }
    if (std::rename(tmp.c_str(), path.c_str()) != 0) {
      throw std::runtime_error("LocalMap::saveCheckpoint: cannot rename " + tmp + " to " + path);
    }
  }
  void loadCheckpoint(const std::string & path)
  {
    requireCheckpoint("loadCheckpoint");
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) {throw std::runtime_error("LocalMap::loadCheckpoint: cannot read " + path);}
    const std::streamoff size = in.tellg();
    std::vector<char> data(size > 0 ? static_cast<size_t>(size) : 0);
    in.seekg(0);
    if (!data.empty() && !in.read(data.data(), static_cast<std::streamsize>(data.size()))) {
      throw std::runtime_error("LocalMap::loadCheckpoint: cannot read " + path);
    }
    uint64_t total = 0;
    uint32_t flags = 0;
    double voxel = 0.0;
    if (data.size() >= VGICP_CHECKPOINT_HEADER_BYTES) {
      std::memcpy(&total, data.data() + 16, 8);
      std::memcpy(&voxel, data.data() + 24, 8);
      std::memcpy(&flags, data.data() + 64, 4);
    }
    if (total < VGICP_CHECKPOINT_HEADER_BYTES || total > data.size()) {
      throw std::runtime_error("LocalMap::loadCheckpoint: " + path + " holds no whole checkpoint");
    }
    // the trailer, if there is one, in full
    uint64_t n = 0;
    const bool trailer = data.size() > total;
    if (trailer) {
      const size_t rest = data.size() - static_cast<size_t>(total);
      if (rest < 16 || std::memcmp(data.data() + total, "VGICPTRJ", 8) != 0) {
        throw std::runtime_error("LocalMap::loadCheckpoint: " + path + " has no trajectory trailer behind the checkpoint");
      }
      std::memcpy(&n, data.data() + total + 8, 8);
      if (n > (rest - 16) / 128 || rest != 16 + 128 * (static_cast<size_t>(n) + 1)) {
        throw std::runtime_error("LocalMap::loadCheckpoint: the trajectory trailer of " + path + " is cut short");
      }
    }
    if (((flags & VGICP_CHECKPOINT_RAW_POINTS) != 0) != rawOnDevice_) {
      throw std::invalid_argument("LocalMap::loadCheckpoint: the checkpoint's raw-points flag is not this map's rawPointsOnDevice");
    }
    if (!(voxel == voxelSize_)) {
      throw std::invalid_argument("LocalMap::loadCheckpoint: the checkpoint's voxel_size is not this map's voxelSize");
    }
    shim::check(ctx_, vgicp_map_restore(ctx_, data.data(), static_cast<size_t>(total), nullptr), "vgicp_map_restore");
    if (!trailer) {return;}
    const auto poseAt = [&data, total](uint64_t i) {
        double m[16];
        std::memcpy(m, data.data() + total + 16 + 128 * i, 128);
        Isometry3d pose = Isometry3d::Identity();
        for (int c = 0; c < 4; ++c) {
          for (int r = 0; r < 4; ++r) {pose.matrix()(r, c) = m[4 * c + r];}
        }
        return pose;
      };
    trajectory_.clear();
    for (uint64_t i = 0; i < n; ++i) {trajectory_.push_back(poseAt(i));}
    prevTransform_ = poseAt(n);
    hasPrevTransform_ = n > 0;
  }
  const std::vector<Isometry3d> & trajectory() const {return trajectory_;}
  const Isometry3d & prevTransform() const {return prevTransform_;}

  // The ray report (include/vgicp_hip_map_rays.h): the first map voxel on every ray of the resident scan at a pose,
  // read-only — which returns appeared in front of the map's surface (VGICP_RAY_BEHIND), which rays the map blocks
  // (VGICP_RAY_BLOCKED: what carving would see through), per point and counted.  Like ICP::pointReport and carveTotals a
  // query beside the drop-in calls: none of them changes its route.  available == false, and nothing thrown, where the
  // map or the scan is not on the device (a host-authoritative map, no resident scan, a module without the library).
  using RayParams = vgicp_ray_params;
  struct RayCounts
  {
    uint64_t rays = 0, visits = 0;
    uint64_t byClass[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // [VGICP_RAY_NO_RAY] .. [VGICP_RAY_NEAR]
  };
  struct RayReport
  {
    bool available = false;
    std::vector<uint8_t> status;      // VGICP_RAY_*, one per point of the resident scan
    std::vector<double> range;        // metres to the hit; NaN with none
    std::vector<int32_t> hitKey;      // 3 per point; INT32_MIN with none
    std::vector<uint32_t> steps;      // voxels visited
    RayCounts counts;
  };
  struct RayCountsList
  {
    bool available = false;
    std::vector<RayCounts> counts;    // one per transform
  };
  RayReport rayReport(const Isometry3d & transform, const RayParams & params) const
  {
    RayReport r;
    if (!deviceResident_ || !vgicp_rays_resident) {return r;}
    size_t n = 0;
    if (vgicp_scan_download(ctx_, 0, nullptr, nullptr, &n) != VGICP_OK) {return r;}   // size query: no resident scan
    r.status.resize(n);
    r.range.resize(n);
    r.hitKey.resize(3 * n);
    r.steps.resize(n);
    const vgicp_ray_outputs out = {r.status.data(), r.range.data(), r.hitKey.data(), r.steps.data()};
    vgicp_ray_counts c;
    const int rc = vgicp_rays_resident(ctx_, shim::poseData(transform), 1, &params, &out, &c, nullptr);
    if (rc == VGICP_ERR_NOT_READY) {return RayReport();}
    shim::check(ctx_, rc, "vgicp_rays_resident");
    r.counts = toRayCounts(c);
    r.available = true;
    return r;
  }
  RayCountsList rayCounts(const std::vector<Isometry3d> & transforms, const RayParams & params) const
  {
    RayCountsList r;
    if (!deviceResident_ || !vgicp_rays_resident || transforms.empty()) {return r;}
    std::vector<double> poses(16 * transforms.size());
    for (size_t k = 0; k < transforms.size(); ++k) {
      std::memcpy(poses.data() + 16 * k, shim::poseData(transforms[k]), 16 * sizeof(double));
    }
    std::vector<vgicp_ray_counts> c(transforms.size());
    const int rc = vgicp_rays_resident(ctx_, poses.data(), transforms.size(), &params, nullptr, c.data(), nullptr);
    if (rc == VGICP_ERR_NOT_READY) {return r;}
    shim::check(ctx_, rc, "vgicp_rays_resident");
    for (const auto & v : c) {r.counts.push_back(toRayCounts(v));}
    r.available = true;
    return r;
  }

private:
  static RayCounts toRayCounts(const vgicp_ray_counts & c)
  {
    RayCounts out;
    out.rays = c.rays;
    out.visits = c.visits;
    for (int k = 0; k < 8; ++k) {out.byClass[k] = c.by_class[k];}
    return out;
  }
  static Key toKey(const Vector3i & v) {return Key{v(0), v(1), v(2)};}
  // the context may have served another map before (shim::defaultContext is shared, and a caller may switch the option
  // through the C ABI): the option is set to THIS map's config every time.  The map is empty here (just reset), which is
  // when the option is accepted; switching it off costs no launch.
  void storeRawPointsOnDevice()
  {
    const bool available = vgicp_set_option && vgicp_map_points_size && vgicp_map_points_export;
    if (!available) {
      if (rawOnDevice_) {
        throw std::runtime_error("LocalMapConfig::rawPointsOnDevice: the linked vgicp module has no raw-point store");
      }
      return;   // a stand-in of the C ABI without the store: nothing to switch off
    }
    shim::check(
      ctx_, vgicp_set_option(ctx_, VGICP_OPTION_MAP_RAW_POINTS, rawOnDevice_ ? 1 : 0),
      "vgicp_set_option(VGICP_OPTION_MAP_RAW_POINTS)");
  }
  void requireCheckpoint(const char * method) const
  {
    const std::string who = std::string("LocalMap::") + method;
    if (!vgicp_map_checkpoint_size || !vgicp_map_checkpoint || !vgicp_map_restore) {
      throw std::runtime_error(who + ": the linked vgicp module has no map checkpoint (libvgicp_hip_map_checkpoint.so)");
    }
    if (!deviceResident_ || (keepRawPoints_ && !rawOnDevice_)) {
      throw std::runtime_error(
              who + ": the map's points live in the host's shadow grid, which a checkpoint does not restore "
              "(deviceResident, and with keepRawPoints also rawPointsOnDevice)");
    }
  }
  static double now()
  {
    return std::chrono::duration<double>(
      std::chrono::steady_clock::now().time_since_epoch()).count();
  }

  // reference: src/LocalMap.cpp:114-118
  Vector3i getVoxelIndex(const Vector3d & point) const
  {
    Vector3i idx;
    for (int a = 0; a < 3; ++a) {idx(a) = static_cast<int>(std::floor(point(a) / voxelSize_));}
    return idx;
  }

  // reference: src/LocalMap.cpp:132-147
  bool needsMapUpdate(const Isometry3d & transform) const
  {
    const Isometry3d moved = prevTransform_.inverse() * transform;
    const auto R = moved.linear();
    const double cosine = 0.5 * (R(0, 0) + R(1, 1) + R(2, 2) - 1.0);
    if (cosine < cosineThreshold_) {return true;}
    const auto t = moved.translation();
    const double translationSq = t(0) * t(0) + t(1) * t(1) + t(2) * t(2);
    if (translationSq > translationSquaredThreshold_) {return true;}
    return false;
  }

  // reference: src/LocalMap.cpp:149-154
  bool needsPointRemoval(const Key & key, const Vector3d & currentPos) const
  {
    const double c[3] = {(key.i + 0.5) * voxelSize_, (key.j + 0.5) * voxelSize_,
      (key.k + 0.5) * voxelSize_};
    const double d0 = c[0] - currentPos(0), d1 = c[1] - currentPos(1), d2 = c[2] - currentPos(2);
    return std::sqrt(d0 * d0 + d1 * d1 + d2 * d2) > distanceThreshold_;
  }

  // The reference's loops over the host grid, once: the host-authoritative map runs them on the caller's thread and
  // listens (which voxels changed, which keys went) for the device mirror; the shadow grid's worker runs them and listens
  // to nothing.
  // src/LocalMap.cpp:47-58; onTouched(key, voxel, changed)
  template<typename OnTouched>
  void insertPoints(const PointCloud & cloud, OnTouched onTouched)
  {
    const auto & points = cloud.points_;
    const auto & covariances = cloud.covariances_;
    for (size_t i = 0; i < points.size(); ++i) {
      const Key key = toKey(getVoxelIndex(points[i]));
      auto found = voxelGrid_.find(key);
      if (found == voxelGrid_.end()) {
        found = voxelGrid_.emplace(key, Voxel(maxNumPointsPerVoxel_, points[i], covariances[i])).first;
        onTouched(key, found->second, true);
      } else {
        onTouched(key, found->second, found->second.addPoint(points[i], covariances[i]));
      }
    }
  }
  // src/LocalMap.cpp:60-72; onErased(key); returns how many voxels went
  template<typename OnErased>
  size_t eraseDistantVoxels(const Vector3d & position, OnErased onErased)
  {
    size_t numRemovedVoxels = 0;
    for (auto it = voxelGrid_.begin(); it != voxelGrid_.end(); ) {
      if (needsPointRemoval(it->first, position)) {
        onErased(it->first);
        it = voxelGrid_.erase(it);
        ++numRemovedVoxels;
      } else {
        ++it;
      }
    }
    return numRemovedVoxels;
  }
  // an eviction that was due is done: the period starts again, and the reference's line (src/LocalMap.cpp:71)
  void evictionDone(size_t numRemovedVoxels)
  {
    currentRemoveTime_ = now();
    std::cout << "removed " << numRemovedVoxels << " voxels\n";
  }
  void evictOnDevice(const Vector3d & position)
  {
    const double pos[3] = {position(0), position(1), position(2)};
    size_t numRemovedVoxels = 0;
    shim::check(ctx_, vgicp_map_evict(ctx_, pos, distanceThreshold_, &numRemovedVoxels), "vgicp_map_evict");
    evictionDone(numRemovedVoxels);
  }
  // The host-authoritative map's insertion (and eviction): the reference's loops on this thread; every voxel they touched
  // goes to the device mirror as ONE upsert batch, every key they erased as ONE erase batch.
  void updateHostMap(const PointCloud & cloud, const Vector3d & position, bool evict)
  {
    std::vector<Voxel *> touched;
    std::vector<Key> touchedKeys;
    insertPoints(
      cloud, [&](const Key & key, Voxel & voxel, bool changed) {
        if (changed && !voxel.dirty) {
          voxel.dirty = true;
          touched.push_back(&voxel);
          touchedKeys.push_back(key);
        }
      });
    std::vector<int32_t> erased;
    if (evict) {
      evictionDone(
        eraseDistantVoxels(
          position, [&](const Key & key) {
            erased.push_back(key.i);
            erased.push_back(key.j);
            erased.push_back(key.k);
          }));
    }
    syncDevice(touched, touchedKeys, erased);
  }

  // ---- the shadow grid's worker (deviceResident + keepRawPoints) --------------------------------------------------
  struct ShadowOp
  {
    PointCloudPtr cloud;
    Isometry3d transform = Isometry3d::Identity();
    bool transformFirst = false;   // the cloud is still in the scan frame (nobody else holds it): move it here
    bool insert = false;
    bool evict = false;
    Vector3d position;
  };
  void shadowApply(ShadowOp & op)
  {
    if (op.cloud && op.transformFirst) {op.cloud->Transform(op.transform.matrix());}
    if (op.cloud && op.insert) {insertPoints(*op.cloud, [](const Key &, Voxel &, bool) {});}
    if (op.evict) {eraseDistantVoxels(op.position, [](const Key &) {});}
    if (op.cloud && op.cloud.use_count() == 1) {shim::recycleStorage(*op.cloud);}   // its last owner: the buffers stay
    op.cloud.reset();
  }
  // what the plan says the worker gets: the caller's cloud or a copy, and what to do with it
  void shadowHandOver(const shim::UpdatePlan & plan, PointCloudPtr & cloud, const Isometry3d & transform)
  {
    ShadowOp op;
    if (plan.handOver == shim::UpdatePlan::HandOver::MoveCloud) {
      op.cloud = std::move(cloud);
    } else {
      op.cloud = std::make_shared<PointCloud>(*cloud);
    }
    op.transform = transform;
    op.transformFirst = plan.transform == shim::UpdatePlan::Transform::OnWorker;
    op.insert = plan.insert;
    op.evict = plan.evict;
    op.position = transform.translation();
    shim::TraceScope tsShadow(shim::Trace::UpdateShadow);
    shadowPush(std::move(op));
  }
  void shadowLoop()
  {
    std::unique_lock<std::mutex> lk(shadowMutex_);
    for (;;) {
      shadowCv_.wait(lk, [&] {return shadowQuit_ || !shadowQueue_.empty();});
      if (shadowQueue_.empty()) {return;}                    // quit, and nothing left to apply
      ShadowOp op = std::move(shadowQueue_.front());
      shadowQueue_.pop_front();
      shadowBusy_ = true;
      lk.unlock();
      shadowApply(op);
      lk.lock();
      shadowBusy_ = false;
      shadowIdle_.notify_all();
    }
  }
  void shadowPush(ShadowOp && op)
  {
    std::unique_lock<std::mutex> lk(shadowMutex_);
    if (!shadowThread_.joinable()) {shadowThread_ = std::thread([this] {shadowLoop();});}
    // at the sensor's rate the worker is idle most of the time; a caller that runs frames back to back faster than the
    // host can file their points waits here rather than let the backlog grow without bound
    shadowIdle_.wait(lk, [&] {return shadowQueue_.size() < 256;});
    shadowQueue_.push_back(std::move(op));
    lk.unlock();
    shadowCv_.notify_one();
  }
  void shadowDrain() const
  {
    std::unique_lock<std::mutex> lk(shadowMutex_);
    shadowIdle_.wait(lk, [&] {return shadowQueue_.empty() && !shadowBusy_;});
  }
  void shadowStop()
  {
    {
      std::lock_guard<std::mutex> lk(shadowMutex_);
      shadowQuit_ = true;
    }
    shadowCv_.notify_all();
    if (shadowThread_.joinable()) {shadowThread_.join();}
  }

  void syncDevice(
    const std::vector<Voxel *> & touched, const std::vector<Key> & keys,
    const std::vector<int32_t> & erased)
  {
    // a voxel both touched and evicted in this update is gone: its Voxel* is dangling, skip by key
    std::vector<int32_t> k;
    std::vector<double> means, covs;
    k.reserve(3 * touched.size());
    means.reserve(3 * touched.size());
    covs.reserve(9 * touched.size());
    for (size_t n = 0; n < touched.size(); ++n) {
      if (!erased.empty() && voxelGrid_.find(keys[n]) == voxelGrid_.end()) {continue;}
      Voxel * v = touched[n];
      v->dirty = false;
      k.push_back(keys[n].i);
      k.push_back(keys[n].j);
      k.push_back(keys[n].k);
      for (int a = 0; a < 3; ++a) {means.push_back(v->mean(a));}
      for (int e = 0; e < 9; ++e) {covs.push_back(v->covariance.data()[e]);}
    }
    if (!erased.empty()) {
      shim::check(ctx_, vgicp_map_erase(ctx_, erased.size() / 3, erased.data()), "vgicp_map_erase");
    }
    if (!k.empty()) {
      shim::check(
        ctx_, vgicp_map_upsert(ctx_, k.size() / 3, k.data(), means.data(), covs.data()),
        "vgicp_map_upsert");
    }
  }

  double voxelSize_;
  size_t maxNumPointsPerVoxel_;
  double translationSquaredThreshold_;
  double cosineThreshold_;
  bool removeDistantPoints_;
  double distanceThreshold_;
  double removePeriod_;
  bool deviceResident_ = false;
  bool keepRawPoints_ = false;
  bool rawOnDevice_ = false;         // the device map keeps the raw points: no shadow grid
  bool shadowComplete_ = true;       // every frame inserted on the device so far has also reached the shadow grid
  double insertGate_ = 0.0;          // > 0: the resident route inserts through the gated entry (setInsertGate)
  uint64_t plainFrames_ = 0;
  bool carve_ = false;               // the resident route carves before it inserts (setCarve)
  int levels_ = 0;                   // coarser levels the device keeps of this map (setLevels)
  vgicp_carve_params carveParams_ = {{0.0, 0.0, 0.0}, 0.0, 0.0, 1, 1};
  std::thread shadowThread_;
  mutable std::mutex shadowMutex_;
  mutable std::condition_variable shadowCv_, shadowIdle_;
  std::deque<ShadowOp> shadowQueue_;
  bool shadowBusy_ = false, shadowQuit_ = false;
  double currentRemoveTime_ = std::numeric_limits<double>::lowest();
  Isometry3d prevTransform_ = Isometry3d::Identity();
  bool hasPrevTransform_ = false;

  VoxelGrid voxelGrid_;

  bool visualize_;
  std::vector<Isometry3d> trajectory_;
  vgicp_ctx * ctx_;
};
}  // namespace ESKF_LIO

#endif  // ESKF_LIO_SHIM_LOCAL_MAP_HPP_
