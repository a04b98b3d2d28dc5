// The shim's robust settings (include/eskf_lio_shim/Registration.hpp: ICP::setRobust, the optional YAML keys
// registration.robust_kernel / robust_scale / gate) on the CPU, against the stand-in headers of tests/compile_native/stubs.
// Built twice: with the stand-in node whose keys are all ABSENT (the reference's own file: the plain round), and with
// -DKEYS_PRESENT and tests/native/yaml_with_keys in front (every key present: "cauchy", 0.125, 0.125).  No call reaches
// the C ABI: nothing here aligns.
#include <cstdio>
#include <stdexcept>

#include "eskf_lio_shim/Registration.hpp"

#if !defined(ESKF_LIO_SHIM_NATIVE_TYPES) || !defined(ESKF_LIO_SHIM_HAVE_YAML)
#error "the native-types branch with YAML was not selected: the stand-in headers are not on the include path"
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
  using ESKF_LIO::RegistrationConfig;
  const YAML::Node config;
  ICP fromYaml(config);
#if defined(KEYS_PRESENT)
  CHECK(fromYaml.robustKernel() == VGICP_ROBUST_CAUCHY && fromYaml.robustScale() == 0.125 && fromYaml.robustGate() == 0.125);
#else
  CHECK(fromYaml.robustKernel() == VGICP_ROBUST_NONE && fromYaml.robustScale() == 1.0 && fromYaml.robustGate() == 0.0);
#endif
  CHECK(RegistrationConfig::robustKernelFromName("none") == VGICP_ROBUST_NONE);
  CHECK(RegistrationConfig::robustKernelFromName("huber") == VGICP_ROBUST_HUBER);
  CHECK(RegistrationConfig::robustKernelFromName("cauchy") == VGICP_ROBUST_CAUCHY);
  CHECK(refuses([] {(void)RegistrationConfig::robustKernelFromName("tukey");}));

  RegistrationConfig c;
  ICP icp(c);
  CHECK(icp.robustKernel() == VGICP_ROBUST_NONE && icp.robustScale() == 1.0 && icp.robustGate() == 0.0);
  icp.setRobust(VGICP_ROBUST_HUBER, 0.08, 0.04);
  CHECK(icp.robustKernel() == VGICP_ROBUST_HUBER && icp.robustScale() == 80000 / 1000000.0 && icp.robustGate() == 40000 / 1000000.0);
  // a bad kind, a scale below a millionth, a negative gate, values beyond an int of millionths: refused, nothing changes
  CHECK(refuses([&] {icp.setRobust(3, 0.1, 0.0);}));
  CHECK(refuses([&] {icp.setRobust(-1, 0.1, 0.0);}));
  CHECK(refuses([&] {icp.setRobust(VGICP_ROBUST_CAUCHY, 0.0, 0.0);}));
  CHECK(refuses([&] {icp.setRobust(VGICP_ROBUST_CAUCHY, 0.1, -0.01);}));
  CHECK(refuses([&] {icp.setRobust(VGICP_ROBUST_CAUCHY, 3000.0, 0.0);}));
  CHECK(refuses([&] {icp.setRobust(VGICP_ROBUST_CAUCHY, 0.1, 3000.0);}));
  CHECK(icp.robustKernel() == VGICP_ROBUST_HUBER && icp.robustScale() == 0.08 && icp.robustGate() == 0.04);
  icp.setRobust(VGICP_ROBUST_HUBER, 2147.483647, 0.0);   // the neutral mode of the tests: INT32_MAX millionths
  CHECK(icp.robustScale() == 2147483647 / 1000000.0);
  c.robustKernel = 9;
  CHECK(refuses([&] {ICP bad(c);}));
  std::printf("ok\n");
  return 0;
}
