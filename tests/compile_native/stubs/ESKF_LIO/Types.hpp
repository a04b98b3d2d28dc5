// STAND-IN for the reference's include/ESKF_LIO/Types.hpp (see ../Eigen/Dense): the filter state and the lidar
// measurement with only the members the shim's native-types branch and the call sites read (the state's time, position
// and attitude; the measurement's cloud and per-point capture times).  It pins NOTHING numerically.
#pragma once
#include <memory>
#include <vector>

#include <Eigen/Dense>
#include <open3d/Open3D.h>

namespace ESKF_LIO
{
using PointCloud = open3d::geometry::PointCloud;
using PointCloudPtr = std::shared_ptr<PointCloud>;

struct LidarMeasurement
{
  PointCloudPtr cloud;
  std::vector<double> pointTime;
  double startTime = 0.0;
  double endTime = 0.0;
};
using LidarMeasurementPtr = std::shared_ptr<LidarMeasurement>;

struct State
{
  double timestamp = 0.0;
  Eigen::Vector3d position = Eigen::Vector3d::Zero();
  Eigen::Vector3d velocity = Eigen::Vector3d::Zero();
  Eigen::Quaterniond attitude = Eigen::Quaterniond::Identity();
};
}  // namespace ESKF_LIO
