// The shim's scale from a quantile of d^2 (include/eskf_lio_shim/Registration.hpp: ICP::robustScaleFromQuantile, beside
// ICP::pointReport) on the CPU, against the stand-in headers of tests/compile_native/stubs.  No call reaches the C ABI:
// vgicp_points_resident is referenced weakly and nothing here links its library, so pointReport itself says so.
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>

#include "eskf_lio_shim/Registration.hpp"

#if !defined(ESKF_LIO_SHIM_NATIVE_TYPES)
#error "the native-types branch was not selected: the stand-in headers are not on the include path"
#endif

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

template <typename F>
static bool refuses(F && f)
{
  try {
    f();
  } catch (const std::invalid_argument &) {
    return true;
  }
  return false;
}

int main()
{
  using ESKF_LIO::ICP;
  // c = factor * sqrt(quantile of d^2): c is compared with d, c^2 with d^2
  CHECK(ICP::robustScaleFromQuantile(0.0625) == 0.25);
  CHECK(ICP::robustScaleFromQuantile(0.0625, 2.0) == 0.5);
  CHECK(ICP::robustScaleFromQuantile(0.066) == std::sqrt(0.066));
  CHECK(ICP::robustScaleFromQuantile(1e-300, 1.0) == std::sqrt(1e-300));
  const double c = ICP::robustScaleFromQuantile(0.0064, 1.0);
  CHECK(std::fabs(c * c - 0.0064) <= 2e-18);
  // the scale goes where setRobust takes it
  ESKF_LIO::RegistrationConfig config;
  ICP icp(config);
  icp.setRobust(VGICP_ROBUST_HUBER, ICP::robustScaleFromQuantile(0.0625), 0.0);
  CHECK(icp.robustScale() == 0.25);
  // refused: a quantile that is NaN (nothing ranked), zero, negative or infinite; a factor that is not positive and finite
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(nan);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(0.0);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(-0.0);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(-0.01);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(inf);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(0.01, 0.0);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(0.01, -1.0);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(0.01, nan);}));
  CHECK(refuses([&] {(void)ICP::robustScaleFromQuantile(0.01, inf);}));
  // a report starts empty
  ICP::PointReport report;
  CHECK(report.points == 0 && report.matched == 0 && report.counted == 0 && report.negative == 0 && report.notFinite == 0);
  CHECK(report.quantiles.empty() && report.d2.empty() && report.squaredError.empty() && report.weight.empty() && report.status.empty());
  CHECK(VGICP_POINT_MATCHED == 1u && VGICP_POINT_NEGATIVE == 2u && VGICP_POINT_NOT_FINITE == 4u);
  std::printf("ok\n");
  return 0;
}
