// The shim's pose prior (include/eskf_lio_shim/Registration.hpp: ICP::setPrior, clearPrior, alignWithPrior,
// posteriorInformation; include/vgicp_hip_prior.h) on the CPU, against the stand-in headers of tests/compile_native/stubs.
// The new members are compiled with their reference-shaped signatures and the bookkeeping that needs no device is run;
// no call reaches the C ABI (its entry points are referenced weakly and nothing here aligns).
#include <cstdio>
#include <type_traits>

#include "eskf_lio_shim/Registration.hpp"

#if !defined(ESKF_LIO_SHIM_NATIVE_TYPES)
#error "the native-types branch was not selected: the stand-in headers are not on the include path"
#endif

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

using ESKF_LIO::ICP;
using ESKF_LIO::Isometry3d;
using ESKF_LIO::LocalMap;
using ESKF_LIO::Matrix6d;
using ESKF_LIO::PointCloud;

// the signatures the issue names (unevaluated: nothing is emitted, so nothing has to link)
static_assert(std::is_same<decltype(&ICP::setPrior), void (ICP::*)(const Isometry3d &, const Matrix6d &)>::value, "setPrior");
static_assert(std::is_same<decltype(&ICP::clearPrior), void (ICP::*)()>::value, "clearPrior");
static_assert(std::is_same<decltype(&ICP::alignWithPrior),
  Isometry3d (ICP::*)(const PointCloud &, const LocalMap &, const Isometry3d &, const Matrix6d &)>::value, "alignWithPrior");
static_assert(std::is_same<decltype(&ICP::posteriorInformation), Matrix6d (ICP::*)() const>::value, "posteriorInformation");
static_assert(std::is_same<decltype(&ICP::align),
  Isometry3d (ICP::*)(const PointCloud &, const LocalMap &, const Isometry3d &)>::value, "align keeps its signature");

int main()
{
  ESKF_LIO::RegistrationConfig c;
  ICP icp(c);
  CHECK(!icp.hasPrior());
  Matrix6d info = Matrix6d::Zero();
  for (int k = 0; k < 6; ++k) {info(k, k) = 10.0 + k;}
  info(1, 0) = info(0, 1) = 0.5;
  CHECK(info.data()[1 + 6 * 0] == 0.5 && info.data()[0 + 6 * 1] == 0.5 && info.data()[5 + 6 * 5] == 15.0);   // column-major
  Isometry3d T;
  icp.setPrior(T, info);
  CHECK(icp.hasPrior());
  icp.setPrior(T, Matrix6d::Zero());   // replaced: still set (the library takes an all-zero information as "no prior")
  CHECK(icp.hasPrior());
  icp.clearPrior();
  CHECK(!icp.hasPrior());
  icp.clearPrior();              // clearing twice is fine
  CHECK(!icp.hasPrior());
  // the robust settings and the prior are independent members
  icp.setRobust(VGICP_ROBUST_CAUCHY, 0.15, 0.06);
  icp.setPrior(T, info);
  CHECK(icp.hasPrior() && icp.robustKernel() == VGICP_ROBUST_CAUCHY);
  // a stand-in of the C ABI without the entry points: the weak references are null here
  CHECK(vgicp_set_pose_prior == nullptr && vgicp_pose_prior_chart == nullptr);
  std::printf("ok\n");
  return 0;
}
