// ResidentScan.hpp — "this host cloud IS the scan that is resident on the device": the stamp CloudPreprocessor::process
// leaves on a cloud, the hash over the cloud's bytes that guards it (16 lanes, AVX2 where the CPU has it, helper threads
// for large clouds), and shim::materialize for a cloud whose prepared scan is on the device only.
#ifndef ESKF_LIO_SHIM_RESIDENT_SCAN_HPP_
#define ESKF_LIO_SHIM_RESIDENT_SCAN_HPP_

#if defined(__x86_64__) && (defined(__GNUC__) || defined(__clang__))
#include <immintrin.h>
#endif
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

#include "ShimSupport.hpp"

namespace ESKF_LIO
{
namespace shim
{
// ---- "this host cloud IS the scan that is resident on the device" --------------------------------------------
// CloudPreprocessor::process leaves the prepared scan on the device and stamps the host cloud; ICP::align and
// LocalMap::updateLocalMap (src/Odometry.cpp:74,79,86 hand the SAME cloud from one to the next) recognise the stamp
// and work on the resident scan instead of uploading the cloud again.  The stamp is the cloud's address, its
// buffers' addresses and sizes, a hash over the buffers' contents and the library's
// scan generation (VGICP_COUNTER_SCAN_GENERATION: anything else that replaced the resident scan voids it).  A
// cloud that was resized, reallocated or edited in place — ANY byte of either buffer: by default every byte is hashed
// (ResidentCheck::FullHash, ~35 GB/s out of the caches: 0.07 ms per check of a 27 000-point prepared cloud) —
// falls back to the upload path, which is what the reference does with every cloud (src/Registration.cpp:11,
// src/LocalMap.cpp:45-58 always read the host cloud).  ResidentCheck::Sampled hashes 64 evenly spaced elements of each
// buffer instead (first and last included): ~1 us, but an edit of an UNSAMPLED element in place is not seen — only for
// callers that never edit a prepared cloud in place, or call shim::forget(cloud) when they do.  Chosen through the
// configuration (CloudPreprocessorConfig::residentCheck — the class that makes the stamp —, YAML key
// cloud_preprocessor.resident_check: sampled), never through the environment; a stamp remembers how it was made, and
// ICP::align / LocalMap::updateLocalMap check it the way it was made.
enum class ResidentCheck {FullHash, Sampled};
struct ResidentStamp
{
  vgicp_ctx * ctx = nullptr;
  const void * cloud = nullptr;
  const void * pointData = nullptr;
  const void * covData = nullptr;
  size_t pointCount = 0, covCount = 0;
  uint64_t hash = 0, generation = 0;
  bool sampled = false;      // the hash covers 64 elements of each buffer only
  bool wantSampled = false;  // what the configuration asked for (ResidentCheck::Sampled); `sampled` is also set for a deferred host copy
  size_t kept = 0;           // points of the resident scan, when known (0 while the preparation has not reported)
  bool hostIsCurrent = false;  // the host buffers hold the prepared scan (false: the raw sweep, the scan is on the device only)
};
inline std::vector<ResidentStamp> & residentStamps()
{
  static std::vector<ResidentStamp> stamps;
  return stamps;
}
// Every byte of a buffer in one pass at the speed the caches deliver it: 16 interleaved lanes of 64-bit words, each a
// pair of running sums (s1 += w; s2 += s1 — position-dependent, so a changed word, a swapped pair or a shifted run all
// show), folded with odd multipliers at the end.  Not cryptographic: a change detector for buffers nobody attacks.
// AVX2 when the CPU has it (four 4-lane vectors), the same lanes in plain C++ otherwise — the same value either way.
#if defined(__x86_64__) && (defined(__GNUC__) || defined(__clang__))
#define ESKF_LIO_SHIM_HASH_AVX2 1
__attribute__((target("avx2"))) inline void lanesAvx2(const uint64_t * w, size_t blocks, uint64_t (&s1)[16], uint64_t (&s2)[16])
{
  __m256i a[4], b[4];
  for (int v = 0; v < 4; ++v) {
    a[v] = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s1 + 4 * v));
    b[v] = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(s2 + 4 * v));
  }
  for (size_t k = 0; k < blocks; ++k, w += 16) {
    for (int v = 0; v < 4; ++v) {
      a[v] = _mm256_add_epi64(a[v], _mm256_loadu_si256(reinterpret_cast<const __m256i *>(w + 4 * v)));
      b[v] = _mm256_add_epi64(b[v], a[v]);
    }
  }
  for (int v = 0; v < 4; ++v) {
    _mm256_storeu_si256(reinterpret_cast<__m256i *>(s1 + 4 * v), a[v]);
    _mm256_storeu_si256(reinterpret_cast<__m256i *>(s2 + 4 * v), b[v]);
  }
}
#endif
// The sums of a run of full 16-word blocks, from zero: A[l] = the lane's words added up, B[l] = its running sums added
// up (= sum of (blocks - k) x word k).  Runs that follow one another combine (blocks' weights shift by what comes after),
// so a buffer can be summed in pieces, on several cores (HashCrew below) or by the device (vgicp_scan_fetch_sums).
struct HashChunk
{
  const uint64_t * w = nullptr;
  size_t blocks = 0;
  uint64_t A[16], B[16];
};
inline void laneSums(HashChunk & c)
{
  for (int l = 0; l < 16; ++l) {c.A[l] = 0; c.B[l] = 0;}
  size_t done = 0;
#ifdef ESKF_LIO_SHIM_HASH_AVX2
  static const bool wide = __builtin_cpu_supports("avx2");
  if (wide) {lanesAvx2(c.w, c.blocks, c.A, c.B); done = c.blocks;}
#endif
  for (size_t k = done; k < c.blocks; ++k) {
    for (size_t l = 0; l < 16; ++l) {
      c.A[l] += c.w[16 * k + l];
      c.B[l] += c.A[l];
    }
  }
}
// consecutive chunks of one buffer -> the sums of all their blocks
inline void combineChunks(const HashChunk * chunks, int count, uint64_t (&A)[16], uint64_t (&B)[16])
{
  for (int l = 0; l < 16; ++l) {A[l] = 0; B[l] = 0;}
  size_t after = 0;
  for (int i = count - 1; i >= 0; --i) {
    for (int l = 0; l < 16; ++l) {
      A[l] += chunks[i].A[l];
      B[l] += chunks[i].B[l] + static_cast<uint64_t>(after) * chunks[i].A[l];
    }
    after += chunks[i].blocks;
  }
}
// the hash of a buffer whose full blocks were summed (A, B): the lanes' start values, the last partial block, the fold
inline uint64_t finishBufferHash(const void * p, size_t bytes, uint64_t seed, const uint64_t (&A)[16], const uint64_t (&B)[16])
{
  const uint64_t * w = static_cast<const uint64_t *>(p);
  const size_t words = bytes / 8, blocks = words / 16;
  uint64_t s1[16], s2[16];
  for (int l = 0; l < 16; ++l) {
    const uint64_t c = seed + 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(l + 1);
    s1[l] = c + A[l];
    s2[l] = static_cast<uint64_t>(blocks) * c + B[l];
  }
  for (size_t i = blocks * 16; i < words; ++i) {
    const size_t l = i & 15u;
    s1[l] += w[i];
    s2[l] += s1[l];
  }
  uint64_t h = bytes * 0x100000001B3ull;
  for (int l = 0; l < 16; ++l) {
    h = (h ^ s1[l]) * 0x9FB21C651E98DF25ull;
    h ^= h >> 29;
    h = (h ^ s2[l]) * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 31;
  }
  return h;
}
inline uint64_t bufferHash(const void * p, size_t bytes, uint64_t seed)
{
  HashChunk c;
  c.w = static_cast<const uint64_t *>(p);
  c.blocks = bytes / 8 / 16;
  laneSums(c);
  return finishBufferHash(p, bytes, seed, c.A, c.B);
}
// A few helper threads that sum chunks beside the caller (or instead of it, while the caller waits for the device): the
// full-hash check reads 96 bytes per point twice a frame, ~70 us each on one core for a 35 000-point scan.  Chunks are
// taken from one atomic word that carries the job's number (a helper that comes late for a job finds the word closed
// or the next job's number and takes nothing); finish() takes what is left itself, so a job ends even when no helper
// ever runs.  Helpers spin for ~100 us after a job (a frame's second check follows its first closely), then sleep.
class HashCrew
{
public:
  static HashCrew & instance()
  {
    static HashCrew crew;
    return crew;
  }
  // how many helper threads jobs may use (0: the caller alone); threads are started when first needed
  void setHelpers(int n) {wanted_.store(n < 0 ? 0 : (n > 3 ? 3 : n), std::memory_order_relaxed);}
  int helpers() const {return wanted_.load(std::memory_order_relaxed);}
  // the chunks' laneSums start on the helpers; finish() must follow (same thread), the chunks stay where they are until then
  void begin(HashChunk * chunks, int count)
  {
    const int want = helpers();
    if (want > static_cast<int>(threads_.size())) {
      std::lock_guard<std::mutex> lk(mutex_);
      while (static_cast<int>(threads_.size()) < want) {threads_.emplace_back([this] {loop();});}
    }
    chunks_.store(chunks, std::memory_order_relaxed);   // (a helper late for the last job may look: its exchange then fails)
    count_.store(count, std::memory_order_relaxed);
    done_.store(0, std::memory_order_relaxed);
    job_ = (job_ + 1u) & 0x7FFFFFFFu;
    ticket_.store(static_cast<uint64_t>(job_) << 32, std::memory_order_seq_cst);     // open, chunk 0 next
    if (want > 0 && sleepers_.load(std::memory_order_seq_cst) > 0) {
      {std::lock_guard<std::mutex> lk(mutex_);}
      wake_.notify_all();
    }
  }
  void finish()
  {
    while (takeOne()) {}
    ticket_.store((static_cast<uint64_t>(job_) << 32) | kClosed, std::memory_order_seq_cst);
    // chunks a helper has taken are being summed (no lock, no device in there): they arrive
    for (uint32_t spins = 0; done_.load(std::memory_order_acquire) != count_.load(std::memory_order_relaxed); ++spins) {
      if (spins < 4096u) {pauseCpu();} else {std::this_thread::yield();}
    }
  }
  ~HashCrew()
  {
    {
      std::lock_guard<std::mutex> lk(mutex_);
      quit_.store(true, std::memory_order_seq_cst);
    }
    wake_.notify_all();
    for (auto & t : threads_) {t.join();}
  }

private:
  static constexpr uint64_t kClosed = 0xFFFFFFFFull;
  static void pauseCpu()
  {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  // one chunk of the open job, if there is one left: summed here
  bool takeOne()
  {
    for (;;) {
      uint64_t t = ticket_.load(std::memory_order_acquire);
      const uint64_t index = t & 0xFFFFFFFFull;
      if (index == kClosed) {return false;}
      HashChunk * chunks = chunks_.load(std::memory_order_relaxed);   // this job's, if the exchange below succeeds (the word
      const int count = count_.load(std::memory_order_relaxed);       //  only changes job when closed)
      if (index >= static_cast<uint64_t>(count)) {return false;}
      if (!ticket_.compare_exchange_weak(t, t + 1u, std::memory_order_acq_rel, std::memory_order_acquire)) {continue;}
      laneSums(chunks[index]);
      done_.fetch_add(1, std::memory_order_release);
      return true;
    }
  }
  void loop()
  {
    for (;;) {
      if (takeOne()) {continue;}
      // nothing to take: watch the word for a while, then sleep until begin() says so
      const uint64_t seen = ticket_.load(std::memory_order_acquire);
      const auto t0 = std::chrono::steady_clock::now();
      bool changed = false;
      for (uint32_t spins = 0; !changed; ++spins) {
        pauseCpu();
        changed = ticket_.load(std::memory_order_acquire) != seen || quit_.load(std::memory_order_relaxed);
        if ((spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(100)) {break;}
      }
      if (quit_.load(std::memory_order_seq_cst)) {return;}
      if (changed) {continue;}
      std::unique_lock<std::mutex> lk(mutex_);
      sleepers_.fetch_add(1, std::memory_order_seq_cst);
      wake_.wait(lk, [&] {return quit_.load(std::memory_order_seq_cst) || ticket_.load(std::memory_order_seq_cst) != seen;});
      sleepers_.fetch_sub(1, std::memory_order_seq_cst);
      if (quit_.load(std::memory_order_seq_cst)) {return;}
    }
  }
  std::mutex mutex_;
  std::condition_variable wake_;
  std::vector<std::thread> threads_;
  std::atomic<uint64_t> ticket_{kClosed};
  std::atomic<int> done_{0}, sleepers_{0}, wanted_{2};
  std::atomic<bool> quit_{false};
  std::atomic<HashChunk *> chunks_{nullptr};
  std::atomic<int> count_{0};
  uint32_t job_ = 0;
};
// sampleHash(cloud, false) in pieces: the chunks of both buffers (points first), summed anywhere, then folded
struct FullHashJob
{
  static constexpr int kMaxChunks = 16;
  HashChunk chunks[kMaxChunks];
  int count = 0, pointChunks = 0;
  const PointCloud * cloud = nullptr;
};
inline void planFullHash(const PointCloud & cloud, FullHashJob & job, int workers)
{
  job.cloud = &cloud;
  job.count = 0;
  const size_t bytesP = cloud.points_.size() * sizeof(Vector3d), bytesC = cloud.covariances_.size() * sizeof(Matrix3d);
  const size_t blocksP = bytesP / 128, blocksC = bytesC / 128;
  // pieces of at least 64 KB, about two per worker so that whoever is faster takes more
  const size_t total = blocksP + blocksC;
  size_t pieces = static_cast<size_t>(workers < 1 ? 1 : workers) * 2;
  const size_t most = total / 512 ? total / 512 : 1;
  pieces = pieces > most ? most : pieces;
  pieces = pieces > static_cast<size_t>(FullHashJob::kMaxChunks - 2) ? static_cast<size_t>(FullHashJob::kMaxChunks - 2) : pieces;
  const size_t per = (total + pieces - 1) / pieces;
  auto cut = [&](const void * p, size_t blocks) {
      const uint64_t * w = static_cast<const uint64_t *>(p);
      size_t at = 0;
      do {
        const size_t take = blocks - at < per + per / 4 ? blocks - at : per;   // no sliver at the end
        HashChunk & c = job.chunks[job.count++];
        c.w = w + 16 * at;
        c.blocks = take;
        at += take;
      } while (at < blocks && job.count < FullHashJob::kMaxChunks - 1);
      if (at < blocks) {job.chunks[job.count - 1].blocks += blocks - at;}
    };
  if (bytesP) {cut(cloud.points_.data(), blocksP);}
  job.pointChunks = job.count;
  if (bytesC) {cut(cloud.covariances_.data(), blocksC);}
}
inline uint64_t foldFullHash(const FullHashJob & job)
{
  const PointCloud & cloud = *job.cloud;
  const size_t n = cloud.points_.size(), m = cloud.covariances_.size();
  uint64_t h = n * 0x100000001B3ull ^ m;
  uint64_t A[16], B[16];
  if (n) {
    combineChunks(job.chunks, job.pointChunks, A, B);
    h = finishBufferHash(cloud.points_.data(), n * sizeof(Vector3d), h, A, B);
  }
  if (m) {
    combineChunks(job.chunks + job.pointChunks, job.count - job.pointChunks, A, B);
    h = finishBufferHash(cloud.covariances_.data(), m * sizeof(Matrix3d), h, A, B);
  }
  return h;
}
// The same value from sums the DEVICE made while it wrote the buffer (vgicp_scan_fetch_sums): a lane that starts at c
// and adds m words ends with s1 = c + A and s2 = m c + B, A the sum of its words and B the sum of (m - k) x word.
inline uint64_t bufferHashFromSums(const uint64_t * A, const uint64_t * B, size_t bytes, uint64_t seed)
{
  const size_t words = bytes / 8;
  uint64_t h = bytes * 0x100000001B3ull;
  for (size_t l = 0; l < 16; ++l) {
    const uint64_t c = seed + 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(l + 1);
    const uint64_t m = (words - l + 15u) >> 4;
    h = (h ^ (c + A[l])) * 0x9FB21C651E98DF25ull;
    h ^= h >> 29;
    h = (h ^ (m * c + B[l])) * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 31;
  }
  return h;
}
// sampleHash(cloud, false) of a cloud of n points and n covariances whose bytes the fetch kernel summed
inline uint64_t fullHashFromSums(const uint64_t (&sums)[64], size_t n)
{
  uint64_t h = n * 0x100000001B3ull ^ n;
  if (n) {
    h = bufferHashFromSums(sums, sums + 16, n * sizeof(Vector3d), h);
    h = bufferHashFromSums(sums + 32, sums + 48, n * sizeof(Matrix3d), h);
  }
  return h;
}
inline uint64_t sampleHash(const PointCloud & cloud, bool sampled)
{
  const size_t n = cloud.points_.size(), m = cloud.covariances_.size();
  if (!sampled) {
    HashCrew & crew = HashCrew::instance();
    FullHashJob job;
    const bool shared = crew.helpers() > 0 && (n * sizeof(Vector3d) + m * sizeof(Matrix3d)) >= (256u << 10);
    planFullHash(cloud, job, shared ? crew.helpers() + 1 : 1);
    if (shared) {
      crew.begin(job.chunks, job.count);
      crew.finish();
    } else {
      for (int i = 0; i < job.count; ++i) {laneSums(job.chunks[i]);}
    }
    return foldFullHash(job);
  }
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](const void * p, size_t bytes) {
      const unsigned char * b = static_cast<const unsigned char *>(p);
      for (size_t i = 0; i < bytes; ++i) {h = (h ^ b[i]) * 1099511628211ull;}
    };
  for (size_t k = 0; k < 64 && n; ++k) {mix(&cloud.points_[k * (n - 1) / 63], sizeof(Vector3d));}
  for (size_t k = 0; k < 64 && m; ++k) {mix(&cloud.covariances_[k * (m - 1) / 63], sizeof(Matrix3d));}
  return h;
}
inline uint64_t scanGeneration(vgicp_ctx * ctx)
{
  uint64_t g = 0;
  check(ctx, vgicp_get_counter(ctx, VGICP_COUNTER_SCAN_GENERATION, &g), "vgicp_get_counter");
  return g;
}
inline ResidentStamp * findStamp(vgicp_ctx * ctx)
{
  for (auto & st : residentStamps()) {
    if (st.ctx == ctx) {return &st;}
  }
  return nullptr;
}
inline void stampResident(
  vgicp_ctx * ctx, const PointCloud & cloud, size_t kept, bool hostIsCurrent,
  ResidentCheck how = ResidentCheck::FullHash, const uint64_t * knownFullHash = nullptr)
{
  ResidentStamp * st = findStamp(ctx);
  if (!st) {
    residentStamps().push_back(ResidentStamp{});
    st = &residentStamps().back();
  }
  st->ctx = ctx;
  st->cloud = &cloud;
  st->pointData = cloud.points_.data();
  st->covData = cloud.covariances_.data();
  st->pointCount = cloud.points_.size();
  st->covCount = cloud.covariances_.size();
  // a host cloud that does NOT hold the prepared scan (HostCopy::Deferred: it still holds the raw sweep, and its contract
  // says "materialize before you touch it") has no content the device's copy could be compared with: its stamp guards
  // the object's identity (address, buffers, sizes, 64 samples), whatever the configuration asks for
  st->wantSampled = how == ResidentCheck::Sampled;
  st->sampled = st->wantSampled || !hostIsCurrent;
  // knownFullHash: the full hash of exactly these bytes, made elsewhere (by the device as it delivered them)
  st->hash = knownFullHash && !st->sampled ? *knownFullHash : sampleHash(cloud, st->sampled);
  st->generation = scanGeneration(ctx);
  st->kept = kept;
  st->hostIsCurrent = hostIsCurrent;
}
// The stamp of `cloud` if object, buffers, sizes and the context's scan generation still are what was stamped (the
// cheap part of the check: the contents are NOT looked at), else nullptr.
inline ResidentStamp * residentIdentityOf(vgicp_ctx * ctx, const PointCloud & cloud)
{
  ResidentStamp * st = findStamp(ctx);
  if (!st || st->cloud != &cloud || st->pointData != cloud.points_.data() ||
    st->covData != cloud.covariances_.data() || st->pointCount != cloud.points_.size() ||
    st->covCount != cloud.covariances_.size())
  {
    return nullptr;
  }
  return st->generation == scanGeneration(ctx) ? st : nullptr;
}
// The stamp of `cloud` if it still is the resident scan of ctx, else nullptr.
inline ResidentStamp * residentStampOf(vgicp_ctx * ctx, const PointCloud & cloud)
{
  ResidentStamp * st = residentIdentityOf(ctx, cloud);
  return st && st->hash == sampleHash(cloud, st->sampled) ? st : nullptr;
}
inline void forget(vgicp_ctx * ctx)
{
  if (ResidentStamp * st = findStamp(ctx)) {st->cloud = nullptr;}
}
inline void forget(const PointCloud & cloud)
{
  for (auto & st : residentStamps()) {
    if (st.cloud == &cloud) {st.cloud = nullptr;}
  }
}
// The host buffers of a cloud whose prepared scan lives on the device only (CloudPreprocessorConfig::HostCopy::
// Deferred) are filled now: one synchronisation and one download.  No-op for any other cloud.
inline void materialize(vgicp_ctx * ctx, PointCloud & cloud)
{
  ResidentStamp * st = residentStampOf(ctx, cloud);
  if (!st || st->hostIsCurrent) {return;}
  size_t n = 0;
  check(ctx, vgicp_scan_download(ctx, 0, nullptr, nullptr, &n), "vgicp_scan_download");
  cloud.points_.resize(n);
  cloud.covariances_.resize(n);
  if (n) {
    check(
      ctx, vgicp_scan_download(
        ctx, n, reinterpret_cast<double *>(cloud.points_.data()),
        reinterpret_cast<double *>(cloud.covariances_.data()), &n), "vgicp_scan_download");
  }
  stampResident(ctx, cloud, n, true, st->wantSampled ? ResidentCheck::Sampled : ResidentCheck::FullHash);
}
}  // namespace shim
}  // namespace ESKF_LIO

#endif  // ESKF_LIO_SHIM_RESIDENT_SCAN_HPP_
