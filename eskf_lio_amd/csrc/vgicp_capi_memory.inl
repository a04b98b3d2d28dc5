// vgicp_capi_memory.inl — part of vgicp_capi.hip (one translation unit, cut by concern; see that file).
// Copies between the caller's pageable memory and the device (the page-locked arena, the streaming CPU copies, the
// symmetric-covariance compaction of the scan upload), and WHEN the context's buffers grow: staging area, voxel table
// (rehash), raw-point log, scan, log.  The buffers are owners (vgicp_owned.h): a grow path decides the size (the voxel
// table's and the raw-point log's come from vgicp_map_plan.h) and waits for whatever still reads the old block; alloc()
// frees that block and then allocates, a temporary is a local owner, and a new block is installed by a move.  An error
// return leaves nothing behind.
namespace {

int settle(vgicp_ctx* ctx);         // defined with the scan preparation below
int fetch_insert_totals(vgicp_ctx* ctx);
int settle_scan(vgicp_ctx* ctx);
int settle_insert(vgicp_ctx* ctx);

// ---- copies between the CALLER'S pageable memory and the device -------------------------------------------------
// hipMemcpyAsync registers a pageable range of more than 1 MB with the driver and lets the DMA engine read it in
// place.  That is the fastest way to move a buffer once -- and a trap for a caller that allocates and frees its buffers
// per frame, as the reference does: when such a range is unmapped (free() of anything above glibc's mmap threshold),
// the driver takes ALL queues of the process off the device until the registration is torn down: 20 - 24 ms in which
// nothing runs (profiles/r10_sync_stall.txt: 23 of 30 ten-frame runs saw it; none with a malloc that keeps its memory).
// So copies of 512 KB - 16 MB go through a page-locked arena of the context instead (smaller ones the runtime stages
// itself; larger ones -- a 10 M-voxel map, a 100 k-point scan -- go up directly, once).  VGICP_STAGE_LIMIT=0: never.
constexpr size_t kArenaBytes = 16u << 20, kArenaMin = 512u << 10;
// VGICP_STAGE_LIMIT, read once per process (nullptr: unset); what a value means is its reader's business (0 switches the
// arena and the scan upload's staging off, the scan preparation stages sweeps up to this many bytes)
const size_t* stage_limit_env() {
  static const char* const text = std::getenv("VGICP_STAGE_LIMIT");
  static const size_t value = text ? (size_t)std::atoll(text) : 0;
  return text ? &value : nullptr;
}
bool staging_off() { return stage_limit_env() && *stage_limit_env() == 0; }

// The CPU copy into page-locked staging memory sets the pace of a frame's first phase (the device idles until the sweep
// has arrived).  The destination is read next by the DMA engine, never by this CPU: streaming stores write it without
// first fetching the lines (no read-for-ownership) and without evicting the caller's data from the caches.
// VGICP_STAGE_COPY=memcpy keeps libc's copy.
__attribute__((target("avx2"))) void stage_copy_avx2(char* dst, const char* src, size_t bytes) {
  size_t i = 0;
  // dst is 64-byte aligned at every call site (page-locked buffers, offsets in multiples of 256 bytes)
  for (; i + 128 <= bytes; i += 128) {
    const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i));
    const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 32));
    const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 64));
    const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i + 96));
    _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i), a);
    _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 32), b);
    _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 64), c);
    _mm256_stream_si256(reinterpret_cast<__m256i*>(dst + i + 96), d);
  }
  _mm_sfence();
  if (i < bytes) std::memcpy(dst + i, src + i, bytes - i);
}
// earliest / latest capture time and "is any NaN" of a sweep, as the plain loops  e = t < e ? t : e;  l = t > l ? t : l
// give them (a NaN never replaces anything; a NaN in t[0] stays): vminpd / vmaxpd return their SECOND operand when the
// comparison fails, which is exactly that.  One dependent chain of 60 000 vminsd is 27 us per sweep; eight lanes: 4 us.
__attribute__((target("avx2"))) void time_range_avx2(const double* t, size_t n, double* earliest, double* latest, bool* any_nan) {
  __m256d mn0 = _mm256_set1_pd(t[0]), mn1 = mn0, mx0 = mn0, mx1 = mn0;
  __m256d un = _mm256_cmp_pd(mn0, mn0, _CMP_UNORD_Q);
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    const __m256d a = _mm256_loadu_pd(t + i), b = _mm256_loadu_pd(t + i + 4);
    mn0 = _mm256_min_pd(a, mn0);
    mn1 = _mm256_min_pd(b, mn1);
    mx0 = _mm256_max_pd(a, mx0);
    mx1 = _mm256_max_pd(b, mx1);
    un = _mm256_or_pd(un, _mm256_or_pd(_mm256_cmp_pd(a, a, _CMP_UNORD_Q), _mm256_cmp_pd(b, b, _CMP_UNORD_Q)));
  }
  double lo[8], hi[8];
  _mm256_storeu_pd(lo, mn0); _mm256_storeu_pd(lo + 4, mn1);
  _mm256_storeu_pd(hi, mx0); _mm256_storeu_pd(hi + 4, mx1);
  double e = lo[0], l = hi[0];
  for (int k = 1; k < 8; ++k) { e = lo[k] < e ? lo[k] : e; l = hi[k] > l ? hi[k] : l; }
  bool nan = _mm256_movemask_pd(un) != 0;
  for (; i < n; ++i) { e = t[i] < e ? t[i] : e; l = t[i] > l ? t[i] : l; nan |= !(t[i] == t[i]); }
  *earliest = e; *latest = l; *any_nan = nan;
}
void time_range(const double* t, size_t n, double* earliest, double* latest, bool* any_nan) {
  static const bool wide = __builtin_cpu_supports("avx2");
  if (wide && n >= 16) { time_range_avx2(t, n, earliest, latest, any_nan); return; }
  double e = t[0], l = t[0];
  bool nan = !(t[0] == t[0]);
  for (size_t i = 1; i < n; ++i) { e = t[i] < e ? t[i] : e; l = t[i] > l ? t[i] : l; nan |= !(t[i] == t[i]); }
  *earliest = e; *latest = l; *any_nan = nan;
}
void stage_copy(void* dst, const void* src, size_t bytes) {
  static const bool streaming = __builtin_cpu_supports("avx2") &&
                                !(std::getenv("VGICP_STAGE_COPY") && std::strcmp(std::getenv("VGICP_STAGE_COPY"), "memcpy") == 0);
  if (streaming && (reinterpret_cast<uintptr_t>(dst) & 31u) == 0) stage_copy_avx2(static_cast<char*>(dst), static_cast<const char*>(src), bytes);
  else std::memcpy(dst, src, bytes);
}
// A unit of covariances (cnt x 9 doubles, column-major) into the staging memory of the scan upload: when every one of
// them is bitwise symmetric — c10 == c01, c20 == c02, c21 == c12; every covariance the reference makes is — only the six
// entries c00 c10 c20 c11 c21 c22 are written (48 instead of 72 bytes per point cross the link; pack_arena_kernel
// mirrors them), else the unit is copied whole.  Returns the form for the unit's flag line.
__attribute__((target("avx2"))) bool cov_unit_compact_avx2(char* dst, const char* src, size_t cnt) {
  const double* s = reinterpret_cast<const double*>(src);
  const uint64_t* w = reinterpret_cast<const uint64_t*>(src);
  double* d = reinterpret_cast<double*>(dst);
  uint64_t bad = 0;
  size_t i = 0;
  // two points per turn: 18 doubles in, 12 out = three aligned 32-byte streaming stores (dst is 64-byte aligned and a
  // pair's 96 bytes keep it 32-byte aligned).  No shuffles: every output vector is two or three overlapping unaligned
  // loads blended (the load ports have room; cross-lane permutes were the bottleneck of a first version), and the
  // symmetry test is scalar on the same cache lines.
  // in: A0 .. A8 at s[0..8], B0 .. B8 at s[9..17]; out: A0 A1 A2 A4 | A5 A8 B0 B1 | B2 B4 B5 B8
  for (; i + 2 <= cnt; i += 2, s += 18, w += 18, d += 12) {
    const __m256d o0 = _mm256_blend_pd(_mm256_loadu_pd(s), _mm256_loadu_pd(s + 1), 0x8);
    const __m256d o1 = _mm256_blend_pd(_mm256_loadu_pd(s + 7), _mm256_loadu_pd(s + 5), 0x1);
    const __m256d o2 = _mm256_blend_pd(_mm256_blend_pd(_mm256_loadu_pd(s + 11), _mm256_loadu_pd(s + 12), 0x6), _mm256_loadu_pd(s + 14), 0x8);
    bad |= (w[1] ^ w[3]) | (w[2] ^ w[6]) | (w[5] ^ w[7]) | (w[10] ^ w[12]) | (w[11] ^ w[15]) | (w[14] ^ w[16]);
    _mm256_stream_pd(d, o0);
    _mm256_stream_pd(d + 4, o1);
    _mm256_stream_pd(d + 8, o2);
  }
  if (i < cnt) {   // an odd count: the unit's (the scan's) last point
    bad |= (w[1] ^ w[3]) | (w[2] ^ w[6]) | (w[5] ^ w[7]);
    const uint64_t o[6] = {w[0], w[1], w[2], w[4], w[5], w[8]};
    std::memcpy(d, o, sizeof o);
  }
  _mm_sfence();
  return bad == 0;
}
uint32_t stage_cov_unit(void* dst, const void* src, size_t cnt) {
  static const bool wide = __builtin_cpu_supports("avx2");
  static const bool off = std::getenv("VGICP_UPLOAD_COMPACT") && std::getenv("VGICP_UPLOAD_COMPACT")[0] == '0';   // A/B aid
  if (wide && !off && (reinterpret_cast<uintptr_t>(dst) & 31u) == 0 &&
      cov_unit_compact_avx2(static_cast<char*>(dst), static_cast<const char*>(src), cnt))
    return kArenaCompact;
  stage_copy(dst, src, cnt * 9 * sizeof(double));   // one asymmetric covariance (or no AVX2): the unit as it is
  return kArenaFull;
}
void arena_reset(vgicp_ctx* ctx) {
  ctx->arena_used = 0;
  ctx->pending_out.clear();
}
char* arena_take(vgicp_ctx* ctx, size_t bytes) {
  if (staging_off() || bytes <= kArenaMin || bytes > kArenaBytes - ctx->arena_used) return nullptr;
  if (!ctx->h_arena && ctx->h_arena.alloc(kArenaBytes) != hipSuccess) return nullptr;
  char* p = ctx->h_arena + ctx->arena_used;
  ctx->arena_used += align256(bytes);
  return p;
}
// page-locked memory (hipHostMalloc / vgicp_host_register): the DMA engine reads it in place, nothing to stage
bool is_pagelocked(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
int user_h2d(vgicp_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return VGICP_OK;
  char* p = bytes > kArenaMin && is_pagelocked(src) ? nullptr : arena_take(ctx, bytes);
  if (!p) {
    VG_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return VGICP_OK;
  }
  const size_t piece = 384u << 10;   // each piece travels while the CPU copies the next
  for (size_t off = 0; off < bytes; off += piece) {
    const size_t len = std::min(piece, bytes - off);
    stage_copy(p + off, static_cast<const char*>(src) + off, len);
    VG_HIP(ctx, hipMemcpyAsync(static_cast<char*>(dst) + off, p + off, len, hipMemcpyHostToDevice, ctx->stream));
  }
  return VGICP_OK;
}
// device -> the caller's memory; complete only after the stream has been synchronised AND user_copies_finish ran
int user_d2h(vgicp_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return VGICP_OK;
  char* p = bytes > kArenaMin && is_pagelocked(dst) ? nullptr : arena_take(ctx, bytes);
  if (!p) {
    VG_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return VGICP_OK;
  }
  VG_HIP(ctx, hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ctx->pending_out.push_back({dst, p, bytes});
  return VGICP_OK;
}
void user_copies_finish(vgicp_ctx* ctx) {
  for (const auto& o : ctx->pending_out) std::memcpy(o.dst, o.src, o.bytes);
  ctx->pending_out.clear();
}

int ensure_stage(vgicp_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->d_stage.bytes()) return VGICP_OK;
  VG_HIP(ctx, ctx->d_stage.alloc(bytes + bytes / 2));
  return VGICP_OK;
}

// ctx->d_stage carved into pieces: taken in order, each at a 256-byte boundary.  First every piece's offset and the total
// (for ensure_stage), then stage_at<T>() turns an offset into a pointer.
struct StageLayout {
  size_t total = 0;
  size_t take(size_t bytes) { const size_t at = total; total += align256(bytes); return at; }
};
template <class T> T* stage_at(const vgicp_ctx* ctx, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(ctx->d_stage.get()) + offset); }

// A page-locked buffer of the context's owner thread is replaced by one of `bytes`, its first `zero_bytes` wiped.  *cap is
// zeroed with the old buffer; the caller sets it (in its own unit) once everything that goes with the new one is in place.
template <class T> int grow_pinned(vgicp_ctx* ctx, PinnedBuf<T>* buf, size_t* cap, size_t bytes, size_t zero_bytes, bool mapped = false) {
  *cap = 0;
  VG_HIP(ctx, mapped ? buf->alloc_mapped(bytes) : buf->alloc(bytes));
  if (zero_bytes) std::memset(buf->get(), 0, zero_bytes);
  return VGICP_OK;
}

// A call that is one device's work on a multi-device context: its first sub-context does it, and the error text comes
// back with the status — or, stage_text, stays with the calling thread (vgicp_sweep_stage*: fail_stage keeps it per thread).
template <class Call> int forward_to_first(const vgicp_ctx* ctx, Call call, bool stage_text = false) {
  vgicp_ctx* first = vgicp_multi_api::first(ctx);
  const int rc = call(first);
  if (rc != VGICP_OK && stage_text) g_stage_error_ctx = ctx->id;
  else if (rc != VGICP_OK) ctx->err = first->err;
  return rc;
}

// an empty table as planned (vgicp_map_plan.h) in *out (whatever *out held is freed first)
int alloc_table(vgicp_ctx* ctx, const TableGrowth& plan, DeviceBuf<VoxelRecord>* out) {
  if (plan.too_large) return fail(ctx, VGICP_ERR_TABLE_FULL, "voxel table would exceed 2^32 slots");
  const uint64_t slots = plan.slots;
  const hipError_t e = out->alloc(slots * sizeof(VoxelRecord));
  if (e != hipSuccess)
    return fail(ctx, VGICP_ERR_TABLE_FULL, std::string("hipMalloc(voxel table): ") + hipGetErrorString(e));
  VG_HIP(ctx, launch_table_clear(ctx->stream, *out, slots));
  return VGICP_OK;
}

// ---- the raw-point store (VGICP_OPTION_MAP_RAW_POINTS) ----
RawLog raw_log(const vgicp_ctx* ctx) {
  RawLog r;
  if (ctx->raw_on) {
    r.entries = ctx->d_raw;
    r.capacity = ctx->raw_capacity;
    r.ctr = ctx->d_ins_counters + 4;
  }
  return r;
}

// An empty log of `entries` in place of the current one (the stream is idle as far as the old one goes: the free).
int raw_replace(vgicp_ctx* ctx, uint64_t entries) {
  ctx->raw_capacity = 0;
  ctx->raw_used_upper = 0;
  const hipError_t e = ctx->d_raw.alloc(entries * sizeof(RawPoint));
  if (e != hipSuccess)
    return fail(ctx, VGICP_ERR_TABLE_FULL, std::string("hipMalloc(raw-point log): ") + hipGetErrorString(e));
  ctx->raw_capacity = (uint32_t)entries;
  ctx->raw_broken = false;
  VG_HIP(ctx, hipMemsetAsync(ctx->d_ins_counters + 4, 0, 3 * sizeof(uint32_t), ctx->stream));
  return VGICP_OK;
}
// sized from the map's capacity hint like the table
int raw_reset(vgicp_ctx* ctx) { return raw_replace(ctx, plan_first_raw_log(ctx->raw_hint)); }

// An append that did not fit leaves entries counted that nobody wrote: from then on the store refuses every call that
// would read or extend it, until vgicp_map_reset (or the option switched on again) makes it anew.
int raw_overflowed(vgicp_ctx* ctx) {
  ctx->raw_broken = true;
  return fail(ctx, VGICP_ERR_TABLE_FULL, "raw-point log overflowed: points of the map were not kept (vgicp_map_reset starts it anew)");
}
int raw_refuse_if_broken(vgicp_ctx* ctx) {
  return ctx->raw_on && ctx->raw_broken ? raw_overflowed(ctx) : VGICP_OK;
}

// The log's device words as a synchronisation brought them to the host: the exact fill, and whether an append failed.
int raw_note(vgicp_ctx* ctx, const uint32_t* words) {
  if (!ctx->raw_on) return VGICP_OK;
  ctx->raw_used_upper = std::min<uint64_t>(words[0], ctx->raw_capacity);
  if (words[1] != 0) return raw_overflowed(ctx);
  return VGICP_OK;
}

// Declared BEHIND local owners whose memory enqueued work may touch (so it goes first): an early return waits for the
// stream before they free.
struct StreamIdleOnExit {
  hipStream_t stream;
  bool armed = true;
  ~StreamIdleOnExit() { if (armed) (void)hipStreamSynchronize(stream); }
};

// Room for the points an insertion of n may accept (all of them).  Only when the bound says the log could fill: one
// synchronisation, the live entries (slot FULL) compacted into a fresh log that is twice as large as needed, geometric.
int ensure_raw(vgicp_ctx* ctx, uint64_t n) {
  if (!ctx->raw_on) return VGICP_OK;
  VG_RC(raw_refuse_if_broken(ctx));
  if (!raw_log_needs_compaction(ctx->raw_used_upper, n, ctx->raw_capacity)) return VGICP_OK;
  uint32_t* ctr = ctx->d_ins_counters + 4;
  DeviceBuf<RawPoint> tmp, grown;
  VG_HIP(ctx, tmp.alloc((size_t)ctx->raw_capacity * sizeof(RawPoint)));
  StreamIdleOnExit idle{ctx->stream};
  VG_HIP(ctx, hipMemsetAsync(ctr + 2, 0, sizeof(uint32_t), ctx->stream));
  VG_HIP(ctx, launch_raw_compact(ctx->stream, ctx->d_raw, (uint32_t)std::min<uint64_t>(ctx->raw_used_upper, ctx->raw_capacity),
                                 ctr, ctx->table, ctx->slots, nullptr, tmp, ctx->raw_capacity, ctr + 2));
  VG_HIP(ctx, hipMemcpyAsync(ctx->h_raw_ctr, ctr, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->h_raw_ctr[1] != 0) return raw_overflowed(ctx);
  const uint64_t live = ctx->h_raw_ctr[2];
  const RawGrowth plan = plan_raw_growth(live, n, ctx->raw_capacity);
  const uint64_t cap = plan.capacity;
  if (plan.too_large) return fail(ctx, VGICP_ERR_TABLE_FULL, "raw-point log would exceed 2^31 points");
  VG_HIP(ctx, hipMemcpyAsync(ctr, ctr + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
  if (cap == ctx->raw_capacity) {
    ctx->d_raw = std::move(tmp);
  } else {
    const hipError_t e = grown.alloc(cap * sizeof(RawPoint));
    if (e != hipSuccess)
      return fail(ctx, VGICP_ERR_TABLE_FULL, std::string("hipMalloc(raw-point log): ") + hipGetErrorString(e));
    if (live) {
      VG_HIP(ctx, hipMemcpyAsync(grown, tmp, live * sizeof(RawPoint), hipMemcpyDeviceToDevice, ctx->stream));
      VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    tmp.reset();
    ctx->d_raw = std::move(grown);
    ctx->raw_capacity = (uint32_t)cap;
  }
  idle.armed = false;
  ctx->raw_used_upper = live;
  return VGICP_OK;
}

int reserve_dense(vgicp_ctx* ctx);
// Room for `incoming` new voxels: when plan_table_growth (vgicp_map_plan.h) says so, a table of the size it says.
int ensure_table(vgicp_ctx* ctx, uint64_t incoming) {
  // a growing table leaves its tombstones behind: a deferred carve's are counted first (voxels + tombstones, the sum
  // the plan is made from, is the same before and after)
  if (ctx->carve_pending && plan_table_growth(ctx->table != nullptr, ctx->slots, ctx->voxels, ctx->tombstones,
                                              ctx->insert_pending_upper, incoming).grow)
    VG_RC(settle(ctx));
  const TableGrowth plan = plan_table_growth(ctx->table != nullptr, ctx->slots, ctx->voxels, ctx->tombstones,
                                             ctx->insert_pending_upper, incoming);
  if (!plan.grow) return VGICP_OK;
  const uint64_t slots = plan.slots;
  // the new table; one scratch word per OLD slot between the claim and the write launch (its own allocation: the staging
  // area may hold the batch that made the table grow); with the raw-point store, the log the live entries move to
  DeviceBuf<VoxelRecord> fresh;
  DeviceBuf<uint32_t> claimed;
  DeviceBuf<RawPoint> moved;
  VG_RC(alloc_table(ctx, plan, &fresh));
  // a failure on the way keeps nothing of the new table (what was enqueued is waited for before the three are freed)
  StreamIdleOnExit idle{ctx->stream};
  int rc_raw = VGICP_OK;
  if (ctx->table) {
    if (ctx->voxels > 0) {
      uint32_t* ctr = ctx->d_ins_counters + 4;
      VG_HIP(ctx, claimed.alloc(ctx->slots * sizeof(uint32_t)));
      if (ctx->raw_on) VG_HIP(ctx, moved.alloc((size_t)ctx->raw_capacity * sizeof(RawPoint)));
      VG_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 4 * sizeof(uint32_t), ctx->stream));
      VG_HIP(ctx, launch_rehash(ctx->stream, ctx->table, ctx->slots, fresh, (uint32_t)(slots - 1), ctx->d_counters, claimed));
      // the raw points follow their voxels to the new slots (claimed maps old -> new); the dead ones stay behind
      if (ctx->raw_on) {
        VG_HIP(ctx, hipMemsetAsync(ctr + 2, 0, sizeof(uint32_t), ctx->stream));
        VG_HIP(ctx, launch_raw_compact(ctx->stream, ctx->d_raw, (uint32_t)std::min<uint64_t>(ctx->raw_used_upper, ctx->raw_capacity),
                                       ctr, ctx->table, ctx->slots, claimed, moved, ctx->raw_capacity, ctr + 2));
        VG_HIP(ctx, hipMemcpyAsync(ctr, ctr + 2, sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        VG_HIP(ctx, hipMemcpyAsync(ctx->h_raw_ctr, ctr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      }
      VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
      claimed.reset();
      if (ctx->raw_on) {
        ctx->d_raw = std::move(moved);
        rc_raw = raw_note(ctx, ctx->h_raw_ctr);
      }
    } else if (ctx->raw_on) {   // no voxel left: every entry is dead, and the new table's slots will be claimed afresh
      VG_HIP(ctx, hipMemsetAsync(ctx->d_ins_counters + 4, 0, sizeof(uint32_t), ctx->stream));
      ctx->raw_used_upper = 0;
    }
    VG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  idle.armed = false;
  ctx->table = std::move(fresh);
  ctx->slots = slots;
  ctx->tombstones = 0;
  ++ctx->map_version;
  VG_RC(reserve_dense(ctx));   // the dense copy's storage follows the table's size here, never inside an align
  return rc_raw;
}

int ensure_scan(vgicp_ctx* ctx, size_t n) {
  if (n <= ctx->scan_capacity && ctx->d_scan) return VGICP_OK;
  ctx->d_scan.reset();
  ctx->d_scan_aos.reset();
  ctx->d_memo.reset();
  ctx->scan_capacity = 0;
  size_t cap = std::max<size_t>(n + n / 4, 1024);
  cap = (cap + 63) & ~size_t(63);  // planes stay 512-byte aligned
  VG_HIP(ctx, ctx->d_scan.alloc(cap * kScanPlanes * sizeof(double)));
  VG_HIP(ctx, ctx->d_scan_aos.alloc(cap * kScanPlanes * sizeof(double)));
  VG_HIP(ctx, ctx->d_memo.alloc(cap * 16));
  ctx->scan_capacity = cap;
  return VGICP_OK;
}

// The resident scan is replaced, or a new preparation is enqueued: a fetch opened for the old scan (vgicp_scan_fetch_begin)
// would copy the old bytes, and the checksums of the last fetch describe the old scan.  Both are void from here on.
void forget_fetch(vgicp_ctx* ctx) {
  ctx->fetch_open = false;
  ctx->fetch_sums_valid = false;
}

// A new resident scan begins: room for n points, the old scan's fetch void, and what vgicp_scan_info reports reset — it
// belongs to a PREPARED scan (prep_voxel > 0), not to one that was uploaded or adopted as it came.
int begin_scan(vgicp_ctx* ctx, size_t n, double prep_voxel, bool with_deskew) {
  VG_RC(ensure_scan(ctx, n));
  ++ctx->scan_generation;
  forget_fetch(ctx);
  ctx->scan_ready = false;
  ctx->prep_voxel = prep_voxel;
  ctx->prep_with_deskew = with_deskew;
  ctx->prep_deskewed = ctx->prep_indefinite = 0;
  ctx->scan_deskewed = 0;
  ctx->scan_indefinite = 0;
  ctx->stride = ctx->scan_capacity;
  return VGICP_OK;
}

int ensure_log(vgicp_ctx* ctx, int iterations) {
  if (iterations <= ctx->log_capacity) return VGICP_OK;
  ctx->d_log.reset();
  ctx->h_log.reset();
  ctx->log_capacity = 0;
  // one header row in front of the iterations' rows (vgicp_context.h: d_log_rows, h_log_rows)
  const int cap = std::max(iterations, 128);
  VG_HIP(ctx, ctx->d_log.alloc((size_t)(cap + 1) * kSlots * sizeof(double)));
  VG_HIP(ctx, ctx->h_log.alloc_mapped((size_t)(cap + 1) * kSlots * sizeof(double)));
  VG_HIP(ctx, hipMemset(ctx->d_log, 0, kSlots * sizeof(double)));
  ctx->log_capacity = cap;
  return VGICP_OK;
}
}  // namespace
