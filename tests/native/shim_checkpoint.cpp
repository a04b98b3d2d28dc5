// The shim's checkpoint members (include/eskf_lio_shim/LocalMap.hpp: LocalMap::saveCheckpoint / loadCheckpoint over
// include/vgicp_hip_map_checkpoint.h) on the CPU, against a stand-in of the C ABI whose map is a byte string: the file is
// the blob verbatim and the trailer, written through path + ".tmp"; a load hands the library the blob's bytes alone and
// brings the trajectory and prevTransform_ back; the shadow-grid modes refuse both; a cut file and a blob of the other
// raw-points flag are refused before the library is asked.  argv[1]: where the file goes (it is left there).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "eskf_lio_shim/Registration.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// ---- the C ABI, stubbed ----
struct vgicp_ctx { int unused; };
static vgicp_ctx g_ctx;
static std::vector<std::string> g_calls;
static std::vector<char> g_map;        // what the device map "is": a checkpoint of it is these bytes
static std::vector<char> g_restored;   // what the last restore was handed
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
int vgicp_map_insert_scan(vgicp_ctx*, size_t n, const double*, const double*, const double*, size_t, size_t* new_voxels) {
  note("insert_scan " + std::to_string(n));
  if (new_voxels) *new_voxels = 0;
  return VGICP_OK;
}
int vgicp_map_insert_resident_async(vgicp_ctx*, const double*, size_t) { return VGICP_OK; }
int vgicp_map_evict(vgicp_ctx*, const double*, double, size_t* removed) { if (removed) *removed = 0; return VGICP_OK; }
int vgicp_match(vgicp_ctx*, size_t, const double*, const double*, double*, double*, double*, double*, uint64_t*, size_t* matched) { if (matched) *matched = 0; return VGICP_OK; }
int vgicp_get_counter(const vgicp_ctx*, int, uint64_t* value) { if (value) *value = 0; return VGICP_OK; }
int vgicp_scan_download(vgicp_ctx*, size_t, double*, double*, size_t* n) { if (n) *n = 0; return VGICP_ERR_NOT_READY; }
int vgicp_scan_upload(vgicp_ctx*, size_t, const double*, const double*) { return VGICP_OK; }
int vgicp_align(vgicp_ctx*, size_t, const double*, const double*, const double* guess, const vgicp_params*, double* pose, vgicp_stats*) {
  std::memcpy(pose, guess, 16 * sizeof(double));
  return VGICP_OK;
}
int vgicp_align_resident(vgicp_ctx*, const double* guess, const vgicp_params*, double* pose, vgicp_stats*) {
  std::memcpy(pose, guess, 16 * sizeof(double));
  return VGICP_OK;
}
int vgicp_align_resident_batch(vgicp_ctx*, size_t, const double*, const vgicp_params*, double*, vgicp_batch_stats*) { return VGICP_OK; }
int vgicp_align_batch_width(vgicp_ctx*, size_t* w) { if (w) *w = 1; return VGICP_OK; }
int vgicp_evaluate_resident(vgicp_ctx*, size_t, const double*, vgicp_evaluation*, vgicp_eval_stats*) { return VGICP_OK; }
int vgicp_map_checkpoint_size(vgicp_ctx*, size_t* bytes) { note("checkpoint_size"); *bytes = g_map.size(); return VGICP_OK; }
int vgicp_map_checkpoint(vgicp_ctx*, size_t capacity, void* blob, size_t* written, vgicp_checkpoint_stats*) {
  note("checkpoint " + std::to_string(capacity));
  *written = g_map.size();
  if (capacity < g_map.size()) return VGICP_ERR_BAD_ARGUMENT;
  std::memcpy(blob, g_map.data(), g_map.size());
  return VGICP_OK;
}
int vgicp_map_restore(vgicp_ctx*, const void* blob, size_t bytes, vgicp_checkpoint_stats*) {
  note("restore " + std::to_string(bytes));
  g_restored.assign(static_cast<const char*>(blob), static_cast<const char*>(blob) + bytes);
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
static std::vector<char> slurp(const std::string & path)
{
  std::ifstream in(path, std::ios::binary);
  return std::vector<char>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
static void spill(const std::string & path, const std::vector<char> & data)
{
  std::ofstream out(path, std::ios::binary | std::ios::trunc);
  out.write(data.data(), static_cast<std::streamsize>(data.size()));
}

int main(int argc, char ** argv) {
  using namespace ESKF_LIO;
  CHECK(argc == 2);
  const std::string path = argv[1];
  // a "blob": a header's worth of bytes whose total_bytes is its length, and a payload
  g_map.assign(128 + 40, 0);
  std::memcpy(g_map.data(), "VGICPMAP", 8);
  const uint64_t total = g_map.size();
  std::memcpy(g_map.data() + 16, &total, 8);
  for (size_t i = 128; i < g_map.size(); ++i) {g_map[i] = static_cast<char>(i * 7);}

  LocalMapConfig onDevice;
  std::memcpy(g_map.data() + 24, &onDevice.voxelSize, 8);   // the blob's voxel_size: the map's
  onDevice.deviceResident = true;
  onDevice.keepRawPoints = false;
  LocalMap map(onDevice, false, &g_ctx);
  for (int f = 1; f <= 3; ++f) {
    auto cloud = std::make_shared<PointCloud>();
    cloud->points_.assign(4, Vector3d());
    cloud->covariances_.assign(4, Matrix3d());
    Isometry3d pose = Isometry3d::Identity();
    pose.matrix()(0, 3) = static_cast<double>(f);
    map.updateLocalMap(cloud, pose, f == 1);
  }
  CHECK(map.trajectory().size() == 3);
  Isometry3d last = Isometry3d::Identity();
  last.matrix()(0, 3) = 9.0;
  {   // prevTransform_ is the last update's pose whether it inserted or not: move it apart from the trajectory's end
    auto cloud = std::make_shared<PointCloud>();
    cloud->points_.assign(1, Vector3d());
    cloud->covariances_.assign(1, Matrix3d());
    map.updateLocalMap(cloud, last, false);
  }
  const size_t frames = map.trajectory().size();   // 4: every update is recorded
  CHECK(frames == 4 && map.prevTransform().matrix()(0, 3) == 9.0);

  // ---- save: the blob verbatim, the trailer, through path + ".tmp"
  g_calls.clear();
  map.saveCheckpoint(path);
  CHECK(g_calls.size() == 2 && g_calls[0] == "checkpoint_size" && g_calls[1] == "checkpoint 168");
  const std::vector<char> file = slurp(path);
  CHECK(file.size() == g_map.size() + 16 + 128 * (frames + 1));
  CHECK(std::memcmp(file.data(), g_map.data(), g_map.size()) == 0);
  CHECK(std::memcmp(file.data() + g_map.size(), "VGICPTRJ", 8) == 0);
  CHECK(slurp(path + ".tmp").empty());

  // ---- load into a second map: the library gets the blob's bytes alone; the trajectory and prevTransform_ are back
  LocalMap second(onDevice, false, &g_ctx);
  CHECK(second.trajectory().empty());
  g_calls.clear();
  second.loadCheckpoint(path);
  CHECK(g_calls.size() == 1 && g_calls[0] == "restore 168" && g_restored == g_map);
  CHECK(second.trajectory().size() == frames && second.prevTransform().matrix()(0, 3) == 9.0);
  for (size_t t = 0; t < frames; ++t) {
    CHECK(std::memcmp(shim::poseData(second.trajectory()[t]), shim::poseData(map.trajectory()[t]), 128) == 0);
  }
  CHECK(std::memcmp(shim::poseData(second.prevTransform()), shim::poseData(map.prevTransform()), 128) == 0);
  // a second save of the loaded map is the same file
  second.saveCheckpoint(path + ".again");
  CHECK(slurp(path + ".again") == file);
  std::remove((path + ".again").c_str());
  // a bare blob (what Python writes): loaded, the trajectory stays
  spill(path + ".bare", g_map);
  g_calls.clear();
  second.loadCheckpoint(path + ".bare");
  CHECK(g_calls.size() == 1 && second.trajectory().size() == frames);
  std::remove((path + ".bare").c_str());

  // ---- refused before the library is asked
  g_calls.clear();
  std::vector<char> cut(file.begin(), file.begin() + 100);
  spill(path + ".cut", cut);
  CHECK(throws<std::runtime_error>([&] {second.loadCheckpoint(path + ".cut");}));
  cut.assign(file.begin(), file.begin() + 150);                       // shorter than total_bytes
  spill(path + ".cut", cut);
  CHECK(throws<std::runtime_error>([&] {second.loadCheckpoint(path + ".cut");}));
  cut.assign(file.begin(), file.end() - 8);                           // the trailer cut short
  spill(path + ".cut", cut);
  CHECK(throws<std::runtime_error>([&] {second.loadCheckpoint(path + ".cut");}));
  cut = file;
  cut[g_map.size()] = 'X';                                            // no trailer magic
  spill(path + ".cut", cut);
  CHECK(throws<std::runtime_error>([&] {second.loadCheckpoint(path + ".cut");}));
  cut = file;
  cut[64] = 1;                                                        // a blob of a map that keeps raw points
  spill(path + ".cut", cut);
  CHECK(throws<std::invalid_argument>([&] {second.loadCheckpoint(path + ".cut");}));
  cut = file;
  const double other = onDevice.voxelSize * 2.0;                      // a blob of another resolution
  std::memcpy(cut.data() + 24, &other, 8);
  spill(path + ".cut", cut);
  CHECK(throws<std::invalid_argument>([&] {second.loadCheckpoint(path + ".cut");}));
  std::remove((path + ".cut").c_str());
  CHECK(throws<std::runtime_error>([&] {second.loadCheckpoint(path + ".missing");}));
  CHECK(g_calls.empty() && second.trajectory().size() == frames);

  // ---- the shadow-grid modes refuse both
  LocalMapConfig shadow;            // deviceResident with keepRawPoints and no rawPointsOnDevice: the default
  CHECK(shadow.deviceResident && shadow.keepRawPoints && !shadow.rawPointsOnDevice);
  LocalMap shadowMap(shadow, false, &g_ctx);
  LocalMapConfig host;
  host.deviceResident = false;
  LocalMap hostMap(host, false, &g_ctx);
  g_calls.clear();
  CHECK(throws<std::runtime_error>([&] {shadowMap.saveCheckpoint(path + ".no");}) && throws<std::runtime_error>([&] {shadowMap.loadCheckpoint(path);}));
  CHECK(throws<std::runtime_error>([&] {hostMap.saveCheckpoint(path + ".no");}) && throws<std::runtime_error>([&] {hostMap.loadCheckpoint(path);}));
  CHECK(g_calls.empty() && slurp(path + ".no").empty());
  std::printf("ok frames %zu bytes %zu\n", frames, file.size());
  return 0;
}
