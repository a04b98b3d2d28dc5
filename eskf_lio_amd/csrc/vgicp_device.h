// vgicp_device.h — device-side data layout and kernel launch entry points (gfx950 only).
//
// HBM layout (DESIGN.md "Data layout"):
//   scan      12 SoA planes of `stride` doubles: x y z c00 c10 c20 c01 c11 c21 c02 c12 c22
//             (a point costs 96 B per iteration, every load is a coalesced 512-B wave access)
//   table     open-addressing hash table of 128-byte voxel records, power-of-two slot count,
//             linear probing, load <= 1/4: a lookup is one cache line, a hit needs no second hop
//   rows      two buffers of one 256-byte row of 32 doubles per workgroup (21 JTJ + 6 JTr + count +
//             4 pad): launch j writes buffer j&1 and folds buffer (j+1)&1 in its prologue
//   state     two AlignStates (ping-pong like the rows): total pose, thresholds, iteration counter,
//             done/converged flags
//   log       per-iteration 32-double rows (reduced normal equations + count), read back once
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "vgicp_launch_plan.h"
#include "vgicp_math.h"

namespace vgicp {

constexpr int kSlots = 32;      // doubles per partial row
constexpr int kNormalEq = 27;   // 21 lower-triangle JTJ entries + 6 JTr entries
constexpr int kCountSlot = 27;  // match count travels as an exact double
constexpr int kCostSlot = 28;     // evaluate_kernel only: sum of e^T (R C R^T + C_voxel)^-1 e
constexpr int kSqErrorSlot = 29;  // evaluate_kernel only: sum of |e|^2
constexpr int kScanPlanes = 12;
constexpr int kMaxIterBlocks = 512;  // grid cap (every workgroup folds all rows: keep them few); larger scans grid-stride

enum : int32_t { SLOT_EMPTY = 0, SLOT_FULL = 1, SLOT_TOMB = 2, SLOT_LOCKED = 3 };

// One voxel of the reference's LocalMap::Voxel as the path reads it: key, mean, covariance
// (reference include/ESKF_LIO/LocalMap.hpp:63-70; numPoints / points stay on the host).
struct alignas(128) VoxelRecord {
  int32_t key[3];
  int32_t state;
  double mean[3];
  double cov[9];  // column-major
  uint64_t count;     // numPoints of the reference's Voxel (device-side insertion freezes it at the cap)
  uint64_t reserved;
};
static_assert(sizeof(VoxelRecord) == 128, "one voxel = one 128-byte line");

struct AlignState {
  double pose[12];  // total transform: R column-major (9) then t (3)
  double step[12];  // last increment
  double cosine_threshold;
  double translation_sq_threshold;
  int32_t max_iteration;
  int32_t iteration;  // rounds executed so far
  int32_t done;       // set on convergence or when iteration == max_iteration
  int32_t converged;
  uint32_t seq;       // persistent launch: echo of PersistArgs::seq, written last (0 from the per-launch loop)
  uint32_t pad;
  // persistent launch only (the host zeroes both before the launch)
  uint32_t abort_seq; // = PersistArgs::seq when ANY workgroup gave up waiting (whatever workgroup 0 concluded)
  uint32_t outcome;   // workgroup 0's verdict: kOutcome*
  // fused align only: device constant-clock ticks (s_memrealtime) from the moment the last workgroup had its staged
  // points in LDS to workgroup 0's commit, the launch's device time without the upload it waited for
  uint64_t unit_to_end_ticks;
};
// AlignState::outcome of a persistent launch
constexpr uint32_t kOutcomeNone = 0;         // workgroup 0 gave up inside a round (or never ran)
constexpr uint32_t kOutcomeCommitted = 1;    // the loop ran to its end (several GPUs: on every rank)
constexpr uint32_t kOutcomeAgreedAbort = 2;  // several GPUs: some rank gave up, every rank knows it
constexpr uint32_t kOutcomeNoAgreement = 3;  // several GPUs: a peer's verdict never arrived

// The resident scan and the voxel map as every launch over them sees them: the base of the five argument structs below
// (resident_view(ctx), vgicp_context.h, fills it).  asym_dev / scan_seq stay fields of each struct (of PoseView for the
// two that share their first 148 bytes), where they always were: a kernel's scalar argument loads are grouped by
// offset, so no field of an argument struct may move (the static_asserts behind each struct hold the offsets).
#pragma GCC diagnostic push   // offsetof in a struct with a base: conditionally supported, and supported by both compilers
#pragma GCC diagnostic ignored "-Winvalid-offsetof"
struct ResidentView {
  const double* scan;  // SoA planes
  uint64_t stride;
  uint32_t n;          // points of the scan
  uint32_t mask;       // slots - 1
  const VoxelRecord* table;
  double voxel_size;
};
static_assert(sizeof(ResidentView) == 40, "the view is the first 40 bytes of every argument struct");
// The view at a pose: the first 148 bytes of PointArgs and GateArgs, what point_term (vgicp_kernels.hip) reads
// (pose_view(ctx, pose16), vgicp_capi_resident.inl, fills it).  A class with a base gives up its tail padding to the
// class derived from it: the field behind scan_seq sits at 148, where it sat in the flat structs.
struct PoseView : ResidentView {
  double pose[12];           // R column-major (9), t (3)
  const uint32_t* asym_dev;  // as IterArgs
  uint32_t scan_seq;
};
static_assert(sizeof(PoseView) == 152 && offsetof(PoseView, pose) == 40, "PoseView: no field may move");
// The robust round (include/vgicp_hip_robust.h) as the kernels take it (robust_args(ctx)); all zero = the plain round
// (vgicp_accumulate, a group's loop, the fused and the team launch: always).
struct RobustArgs {
  uint32_t kernel;   // VGICP_ROBUST_*
  double scale2;     // c^2
  double gate;       // gate on d^2; 0 = none
};
// The pose prior (include/vgicp_hip_prior.h) as the kernels take it (prior_args(ctx)); all zero = no prior (likewise).
struct PriorArgs {
  uint32_t on;
  double pose[12];   // R0 column-major (9) then t0 (3)
  double info[21];   // lower triangle of the information matrix, row by row, as normal_eq is laid out
};

struct IterArgs : ResidentView {
  double* rows;        // [grid][kSlots]: partial rows this launch writes
  const double* prev;  // rows the previous launch wrote (or the all-reduced single row)
  uint32_t prev_rows;  // how many; 0 = first round, nothing to solve yet
  uint32_t pad;
  const AlignState* state_in;
  AlignState* state_out;
  double* log;        // [max_iteration][kSlots]
  uint64_t* stamps;   // diagnostic aid (VGICP_DEBUG_STAMPS=1): phase times of workgroup 0 in 10 ns
                      // ticks, summed over launches; nullptr in normal operation
  // round 6: what the persistent launch keeps on chip, kept in HBM between the launches of one align
  int4* memo;               // [n] per point: voxel key of the last round + its record's slot (index in `dense` when that
                            // is set) / kMemoMiss; written by the launch that finds a point's key changed (all points in
                            // an align's first launch), nullptr = look every point up in every launch
  uint32_t memo_valid;      // != 0: an earlier launch of THIS align filled the memos
  uint32_t scan_seq;        // with asym_dev: *asym_dev != scan_seq = every covariance of the scan is bitwise symmetric
  const uint32_t* asym_dev; // (nine planes are read instead of twelve); nullptr = unknown, read all
  const VoxelRecord* dense; // dense copy of the FULL records (tables beyond the caches' reach), or nullptr
  RobustArgs robust;
  PriorArgs prior;
};
static_assert(sizeof(IterArgs) == 424 && offsetof(IterArgs, rows) == 40 && offsetof(IterArgs, asym_dev) == 112 &&
              offsetof(IterArgs, robust) == 128 && offsetof(IterArgs, prior) == 152, "IterArgs: no field may move");

// Arguments of the persistent single-launch align (single GPU): every round of the loop runs inside
// one kernel.  Workgroups exchange their partial rows through `rows` and `parts` (three buffers each, by
// round modulo 3) with no flag and no counter: every 8-byte word of a buffer holds the bit pattern
// kRowUnset until its producer stores the value (one write-through 8-byte store per word, never torn), and
// consumers poll the words themselves.  Two levels, in the summation order of iterate_kernel<512>:
//   rows   [3][256][kSlots]      workgroup b's sums of the round (21 + 6 + count) at row (b % 16) * 16 + b / 16
//   parts  [3][kFolders][kSlots] folder g (= workgroup g < kFolders) adds the rows b = g, g + 16, g + 32 ...
//                                in ascending order; every workgroup then adds the parts in ascending g
// A producer re-arms its word (stores kRowUnset) one round after everyone has consumed it and two rounds
// before it is written again; DESIGN.md section 4 has the ordering argument.
constexpr int kExchangeRows = 256;                          // 16 folders x 16 rows: the largest persistent grid
constexpr int kMaxRanks = 16;                               // mailbox rows; = kFolders so one poll routine serves both
constexpr int kFolders = 16;                                // = 512 / kSlots, the groups of iterate_kernel<512>'s fold
constexpr unsigned long long kRowUnset = ~0ull;             // a NaN pattern no fp64 operation produces
constexpr unsigned long long kRowNaN = 0x7FF8000000000000ull;  // what a computed NaN is published as
constexpr size_t kMailRowWords = 3 * (size_t)kMaxRanks * kSlots;  // the rows of a mailbox
constexpr size_t kMailWords = kMailRowWords + kSlots;          // + the verdict words (kMaxRanks used)
struct PersistArgs : ResidentView {   // n: an UPPER BOUND when n_dev is set (the launch plan is made from it)
  double* rows;         // [3][kExchangeRows][kSlots]; kRowUnset where a workgroup publishes (between launches: all but the
                        // buffer of the last round, which the next launch's first round re-arms), else +0.0
  double* parts;        // [3][kFolders][kSlots], likewise
  AlignState* state;    // out: final state; state->seq == seq tells the host the loop ran to its end
  double* log;          // [max_iteration][kSlots]
  uint32_t spin_limit;  // an in-kernel wait longer than this many polls gives up (host falls back to launches)
  uint32_t seq;
  // inputs travel with the dispatch packet: no host-to-device copy and no memset per align
  double pose0[12];     // guess: R column-major (9) then t (3)
  double cosine_threshold;
  double translation_sq_threshold;
  int32_t max_iteration;
  uint32_t stash_points;   // at most this many extra points per thread are kept in LDS across rounds (scans larger
                           // than the grid); the kernel parks as many of them as fit stash_bytes
  uint32_t memo_points;    // extra points per thread whose last key + table slot are remembered in LDS
  uint32_t round0;         // rounds executed on this context before this launch (mod 3 matters): the exchange
                           // buffers rotate with round0 + it, so a launch leaves nothing to tidy up
  // multi-GPU (world > 1): the rank totals travel through peer-mapped mailboxes, written by the ranks'
  // kernels themselves over xGMI (no host-enqueued collective between launches)
  uint32_t world, rank;
  uint32_t mail_round0;    // rounds all ranks have executed on this communicator before this launch
  uint32_t mail_seq;       // aligns attempted through the mailboxes on this communicator, this one included (same on
                           // every rank, >= 1): the verdict words at the end of a launch carry it
  double* const* mail;     // device array of kMaxRanks pointers; mail[r]: rank r's mailbox as mapped into THIS
                           // process, [3][kMaxRanks][kSlots] words: by round % 3, row = sender rank (rows >=
                           // world hold +0.0 for good), then kMaxRanks VERDICT words (index = sender rank):
                           // mail_seq << 1 | 1 "my loop ran to its end", mail_seq << 1 "I gave up" — written by
                           // workgroup 0 of the sender at the end of its launch, so that all ranks commit an align
                           // or none does
  const uint32_t* asym_dev;  // nullptr, or the word pack_scan_kernel sets to scan_seq when some covariance of the scan is
  uint32_t scan_seq;         // NOT bitwise symmetric; while it differs, the planes above the diagonal are not read
  uint32_t stash_bytes;      // LDS behind the memos that may hold parked points; how many fit depends on the planes
                             // a parked point needs (9 or 12) and on the point-carrying threads (448 or 512)
  const VoxelRecord* dense;  // nullptr, or the FULL records of the table packed densely (launch_table_dense), for tables
                             // far larger than the caches' and TLBs' reach: a record's index there sits in the upper
                             // half of its spare word; a point that stays in its voxel then reads its payload from
                             // this array (1.3 GB at 10M voxels) instead of from the sparse table (8.6 GB)
  const uint32_t* n_dev;   // nullptr, or where the device holds the scan's size (a scan prepared on the device whose
                           // kept count the host has not read yet: no host round trip between preparation and align)
  double prefetch_margin;  // > 0 (only with memo_points == stash_points == 0): a point closer than this many
                           // voxel sizes to a face of its voxel has the neighbour behind that face looked up
                           // into LDS while the workers wait for the exchange
  uint64_t* stamps;
  RobustArgs robust;
  PriorArgs prior;
};
static_assert(sizeof(PersistArgs) == 576 && offsetof(PersistArgs, rows) == 40 && offsetof(PersistArgs, asym_dev) == 232 &&
              offsetof(PersistArgs, robust) == 280 && offsetof(PersistArgs, prior) == 304, "PersistArgs: no field may move");

// The fused align (vgicp_align, one point per thread, one device): the persistent launch is enqueued BEFORE the copy
// threads stage the scan, and every workgroup reads its own 448 points out of the page-locked staging memory as the
// units are published — what pack_arena_kernel reads and writes for them, in the same layout (see that kernel).
struct FusedUpload {
  const char* apts;          // staged points, 24 bytes per point
  const char* acov;          // staged covariances: unit u starts at acov + 72 * u * unit, compact (48 B) or full (72 B)
  const uint32_t* flags;     // flags[16 * u] == seq: unit u is staged; flags[16 * u + 1]: its form (kArenaCompact / kArenaFull)
  uint32_t unit;             // points per unit (pack_arena_unit())
  uint32_t seq;
  uint32_t spin_limit;       // the pack's patience: polls of a unit's flag, and of round 0's exchange
  double* soa;               // out: the 12 SoA planes (PersistArgs::scan), stride PersistArgs::stride
  double* aos_pts;           // out: the device's AoS copy of the scan
  double* aos_cov;
  uint32_t* asym;            // out: = seq when some covariance is not bitwise symmetric
  unsigned long long* unit_clock;  // device word: the latest s_memrealtime at which a workgroup had its points in LDS
};

// The batched align (vgicp_align_resident_batch): several hypotheses, one resident scan, ONE persistent launch.  With one
// point per thread a scan of n points occupies T = ceil(n / 448) workgroups; the launch's workgroups [h T, (h + 1) T)
// are TEAM h and run hypothesis h exactly as the single launch runs it on its first T workgroups, with the team-local
// index vb = blockIdx.x - h T in the place of blockIdx.x.  Workgroups beyond teams x T leave at once.  A team has exchange
// words of its own (PersistArgs::rows / parts point at team 0's):
//   rows   [3][16 U][kSlots], U = ceil(T / 16)   workgroup vb's row at (vb % 16) * U + vb / 16
//   parts  [3][kFolders][kSlots]                 folder g is the team's workgroup vb = g < 16
// The single launch's folders add 16 rows and its workgroups 16 parts, of which those that belong to workgroups without
// points are +0.0; a team has no such workgroups and puts a literal +0.0 into the same positions of the same pairwise
// tree (poll_and_sum's `live`), so every sum has the single launch's bits.  Every word is kRowUnset when a launch starts
// (the host's memset in front of it) and PersistArgs::round0 is 0: the owner of a word changes with T from call to call.
constexpr int kTeamsMax = 16;          // hypotheses per launch
constexpr int kTeamRowsMax = 512;      // rows per buffer over all teams: teams x 16 U <= 480 for every T at a grid of 256
struct TeamArgs {
  uint32_t teams;         // hypotheses of this launch
  uint32_t team_wgs;      // T
  uint32_t folder_rows;   // U
  uint32_t slot_words;    // doubles between the state + log blocks of two hypotheses (PersistArgs::state / log: team 0's)
  uint32_t* abort_word;   // ONE word for the whole launch: = PersistArgs::seq when any workgroup of any team gave up
  double pose0[kTeamsMax][12];
};
constexpr size_t team_rows_words() { return 3 * (size_t)kTeamRowsMax * kSlots; }
constexpr size_t team_parts_words() { return 3 * (size_t)kTeamsMax * kFolders * kSlots; }

// Scoring poses of the resident scan (vgicp_evaluate_resident): launch (rows per pose) x (poses) workgroups write one
// row each, a second launch folds every pose's rows into 32 doubles.  Row budget of one launch pair: kEvalRowBudget.
constexpr int kEvalRowBudget = 4096;   // 1 MiB of rows: 16 poses of the largest geometry below 256 x 448 points, 8 of kMaxIterBlocks rows
struct EvalArgs : ResidentView {
  const double* poses;       // [poses][12], page-locked host memory as the device addresses it: R column-major (9), t (3)
  double* rows;              // [poses][rows per pose][kSlots]
  const uint32_t* asym_dev;  // as IterArgs
  uint32_t scan_seq;
  uint32_t pad;
};
static_assert(sizeof(EvalArgs) == 72 && offsetof(EvalArgs, poses) == 40 && offsetof(EvalArgs, asym_dev) == 56,
              "EvalArgs: no field may move");

// The resident scan at a pose, point by point (vgicp_points_resident, include/vgicp_hip_points.h): one launch writes the
// requested planes (any of them may be nullptr) and, when quantiles are wanted, a 64-bit sort key and the index per
// point; a second, one wave, reads the counts, picks the ranks from the sorted keys and writes the result into
// page-locked memory.  counters: 4 device words, zero before the first launch: matched, counted, negative, not finite.
constexpr int kPointCounters = 4;
constexpr int kPointQuantiles = 16;        // VGICP_POINT_QUANTILES_MAX
constexpr int kPointResultWords = kPointCounters + kPointQuantiles;
struct PointArgs : PoseView {
  uint32_t robust_kernel;    // RobustArgs, flat: the offset is 4 mod 8 (the view's tail), where a RobustArgs member cannot sit
  double robust_scale2;
  double robust_gate;
  double* d2;                // n each, or nullptr
  double* sq_error;
  double* weight;
  uint8_t* status;
  unsigned long long* keys;  // n keys and ...
  uint32_t* idx;             // ... n indices for the sort, or both nullptr
  uint32_t* counters;
};
static_assert(sizeof(PointArgs) == 224 && offsetof(PointArgs, pose) == 40 && offsetof(PointArgs, asym_dev) == 136 &&
              offsetof(PointArgs, robust_kernel) == 148, "PointArgs: no field may move");
struct PointPickArgs {
  const unsigned long long* sorted;  // the n keys in ascending order (n_quantiles > 0)
  const uint32_t* counters;
  uint32_t n;
  uint32_t n_quantiles;
  double q[kPointQuantiles];
  unsigned long long* out;   // page-locked, kPointResultWords: the four counts, then the quantiles' bit patterns
};

// The decision of a gated map insertion (vgicp_map_insert_resident_gated, include/vgicp_hip_map_gated.h): one launch
// forms every point's term at the pose as point_terms_kernel forms it (ONE definition: point_term) and writes one keep
// byte per point: 0 iff the point is matched and not max(raw, 0) <= gate (a NaN or infinite raw fails every gate, +inf
// included).  Read-only on the table; the insertion that claims slots is a later launch.  counters: 3 device words that
// only ever grow (running totals; the host remembers what it has read): matched, refused, not finite.
constexpr int kGateCounters = 3;
struct GateArgs : PoseView {
  uint32_t pad;
  double gate;               // >= 0 or +inf
  uint8_t* keep;             // n
  uint32_t* counters;
};
static_assert(sizeof(GateArgs) == 176 && offsetof(GateArgs, pose) == 40 && offsetof(GateArgs, asym_dev) == 136,
              "GateArgs: no field may move");
#pragma GCC diagnostic pop

// ---- launchers (defined in vgicp_kernels.hip) ----
hipError_t launch_point_terms(hipStream_t s, const PointArgs& args);
hipError_t launch_gate_decide(hipStream_t s, const GateArgs& args);
hipError_t launch_point_pick(hipStream_t s, const PointPickArgs& args);
// Rows of `poses` poses (grid: rows_per_pose x poses workgroups of 512 threads), and their fold into out[poses][kSlots]:
// slots 0-26 the normal equations, 27 the count, 28 the cost, 29 the squared error.
hipError_t launch_evaluate(hipStream_t s, const EvalArgs& args, uint32_t rows_per_pose, uint32_t poses);
hipError_t launch_evaluate_fold(hipStream_t s, const double* rows, uint32_t rows_per_pose, uint32_t poses, double* out);
// The whole ICP::align loop in one launch (512-thread workgroups, at most one per CU).
hipError_t launch_persistent(hipStream_t s, const PersistArgs& args, uint32_t grid);
// The same loop for args.teams hypotheses side by side (single device, one point per thread, no stamps, settled scan).
hipError_t launch_persistent_teams(hipStream_t s, const PersistArgs& args, const TeamArgs& teams, uint32_t grid);
// The same launch with the scan's upload fused into round 0 (single device, args.n <= grid x 448, no stamps).
hipError_t launch_persistent_fused(hipStream_t s, const PersistArgs& args, const FusedUpload& up, uint32_t grid);
// How launch_persistent splits the CU's LDS for a scan of n points on `grid` workgroups: points per
// thread beyond the first that get a memo (last key + slot, 16 B) and that are parked whole (96 B).
void persistent_lds_plan(uint32_t n, uint32_t grid, uint32_t* memo_points, uint32_t* stash_points, uint32_t* stash_bytes,
                         uint32_t lds_budget = 0);
// Sizes (8-byte words) of the rows / parts exchange buffers, and their content between launches.
size_t persistent_rows_words();
size_t persistent_parts_words();
void persistent_exchange_image(uint32_t grid, unsigned long long* rows_words, unsigned long long* parts_words);
// Whether one 512-thread workgroup of the persistent kernel with this much dynamic LDS fits a CU of the
// current device: *max_grid = cu_count then, else 0 (the in-kernel exchange needs every workgroup resident).
hipError_t persistent_prepare_device();  // once per context, on its device: every instantiation may use the whole CU's LDS
hipError_t persistent_max_resident(uint32_t dyn_lds_bytes, int cu_count, uint32_t* max_grid);
// persistent_dyn_lds_bytes, persistent_max_dyn_lds_bytes: vgicp_launch_plan.h
// One VGICP round over the resident scan: prologue folds args.prev and advances the pose, body
// accumulates this round's rows. block = 256 / 512 / 1024 threads per workgroup.
hipError_t launch_iterate(hipStream_t s, const IterArgs& args, uint32_t grid, int block);
// The prologue-only launch that closes the last round (single workgroup).
hipError_t launch_close(hipStream_t s, const IterArgs& args, int block);
// Multi-GPU: fold nrows rows into sums[kSlots] (the 256-byte message of the all-reduce).
hipError_t launch_fold_rows(hipStream_t s, const double* rows, uint32_t nrows, const AlignState* state,
                            double* sums);
// Test hook: solve + exponential + convergence test of one round on given normal equations (one wave).
hipError_t launch_solve_step(hipStream_t s, const double* packed27, double cosine_threshold,
                             double translation_sq_threshold, int force_pivoted, double* out20);
// out[o] = in[perm[o]], o < m, for a scan's AoS arrays (idx / out_idx optional): VGICP_OPTION_REFERENCE_ORDER
hipError_t launch_gather_scan(hipStream_t s, const uint32_t* perm, uint32_t m, const double* pts, const double* covs,
                              const unsigned long long* idx, double* out_pts, double* out_covs, unsigned long long* out_idx);
// asym: one device word that receives seq when a covariance is not bitwise symmetric (PersistArgs::asym_dev)
hipError_t launch_pack_scan(hipStream_t s, const double* points_aos, const double* covs_aos,
                            uint32_t n, double* soa, uint64_t stride, uint32_t* asym, uint32_t seq);
// The same packing straight out of page-locked HOST staging memory that host threads are still filling, unit by unit
// (pack_arena_unit() points each; flags[16 * u] == seq publishes unit u, flags[16 * u + 1] says in which form its
// covariances were staged; wait == false: all there).  Also leaves the AoS copy on the device.  See pack_arena_kernel.
uint32_t pack_arena_unit();
constexpr uint32_t kArenaFull = 2u;      // a unit's covariances as the caller holds them: 72 bytes per point
constexpr uint32_t kArenaCompact = 1u;   // all of them bitwise symmetric: c00 c10 c20 c11 c21 c22, 48 bytes per point
hipError_t launch_pack_arena(hipStream_t s, const void* arena_points, const void* arena_covs, uint32_t n,
                             const uint32_t* flags, bool wait, uint32_t seq, uint32_t spin_limit, double* aos_pts, double* aos_cov,
                             double* soa, uint64_t stride, uint32_t* asym);
// ---- the voxel table's launchers (defined in vgicp_table.hip) ----
hipError_t launch_table_clear(hipStream_t s, VoxelRecord* table, uint64_t slots);
// Pack the FULL records of `table` into `dense` in slot order (128 bytes each) and leave every record's index there in
// the upper half of its spare word.  block_counts: scratch of table_dense_blocks(slots) + 1 words.
uint32_t table_dense_blocks(uint64_t slots);
hipError_t launch_table_dense(hipStream_t s, VoxelRecord* table, uint64_t slots, VoxelRecord* dense, uint64_t dense_capacity,
                              uint32_t* block_counts);
// claimed: scratch of n words (upsert) / old_slots words (rehash): claim launch -> write launch.  A word is the slot
// claimed with kClaimFresh set when the record is new, or kClaimFailed (probe sequence exhausted; rehash: not FULL).
constexpr uint32_t kClaimFresh = 0x80000000u;
constexpr uint32_t kClaimFailed = 0x7FFFFFFFu;
hipError_t launch_upsert(hipStream_t s, VoxelRecord* table, uint32_t mask, uint32_t n,
                         const int32_t* keys, const double* means, const double* covs,
                         uint32_t* counters /* [0] new inserts, [1] failures */, uint32_t* claimed);
hipError_t launch_erase(hipStream_t s, VoxelRecord* table, uint32_t mask, uint32_t n,
                        const int32_t* keys, uint32_t* counters /* [0] erased */);
hipError_t launch_rehash(hipStream_t s, const VoxelRecord* old_table, uint64_t old_slots,
                         VoxelRecord* table, uint32_t mask, uint32_t* counters, uint32_t* claimed);
hipError_t launch_voxel_index(hipStream_t s, const double* points_aos, uint32_t n, double voxel_size,
                              int32_t* keys);
// Correspondence materialisation in ascending point order (three small passes).
hipError_t launch_match(hipStream_t s, const double* points_aos, const double* covs_aos, uint32_t n,
                        const VoxelRecord* table, uint32_t mask, double voxel_size,
                        uint32_t* block_counts, uint32_t* total, double* src_points,
                        double* src_covs, double* map_points, double* map_covs, uint64_t* src_index);
uint32_t match_blocks(uint32_t n);
// ---- vgicp_levels.hip: a coarser level of the map (include/vgicp_hip_map_levels.h) ----
// Level l in `coarse` (coarse_slots all EMPTY before, a power of two, at least twice the finer level's voxels) from level
// l-1 in `fine`: the CLAIM launch (one thread per finer slot) and the FILL launch (eight lanes per slot of the level).
// counters[0] += voxels of the level, counters[1] += probe sequences exhausted.
hipError_t launch_level_build(hipStream_t s, const VoxelRecord* fine, uint64_t fine_slots, VoxelRecord* coarse,
                              uint64_t coarse_slots, uint32_t* counters);
// Locate (include/vgicp_hip_map_locate.h has the rule): two launches.  SCORE, grid (chunks of the points that take part,
// poses): a workgroup makes the keys of its points once, probes the level's table once per point and cell of the window
// and counts in a histogram in LDS, which it then adds to the plane.  BEST, one workgroup per pose: the maximum with the
// lowest index, written as vgicp_locate_best.  The table is only read.
struct LocateArgs {
  const VoxelRecord* table;    // of the level
  uint32_t mask;               // its slots - 1
  uint32_t cells;              // of the window, at most VGICP_LOCATE_MAX_CELLS
  double voxel_size;           // of the level
  const double* points_aos;    // n x 3
  uint32_t n, stride;
  uint32_t participants;       // points with i % stride == 0
  int32_t window[3];           // half-widths
  const double* poses;         // device: 16 per pose, as the ABI lays a transform out
  uint32_t* skipped;           // per pose, zero before
  uint32_t* plane;             // poses x cells, zero before
};
// best: poses x vgicp_locate_best, where the device writes them (page-locked memory)
hipError_t launch_locate(hipStream_t s, const LocateArgs& args, uint32_t poses, void* best);

// ---- vgicp_mapupdate.hip: LocalMap::updateLocalMap's insert / evict loops on the device ----
// Scratch the insertion needs for n points (bytes), and the insertion itself: transform, find-or-claim
// the voxel of every point, order the points of a voxel by scan index, apply the reference's
// constructor / addPoint rule sequentially per voxel. counters[0] receives the number of new voxels.
size_t map_insert_scratch_bytes(uint32_t n);

// vgicp_preprocess.hip — voxel down-sampling + k-NN covariances (CloudPreprocessor.cpp:76-127)
// Words of the context's counter block (device; a copy travels to pinned host memory after a preparation):
//   [0] kept points  [1] octree cells over all levels  [2..7] developer counts  [8..71] developer histograms
//   [72] kept points whose regularised covariance is indefinite (src/CloudPreprocessor.cpp:119-123)
//   [73] = the call's epoch when a point lies beyond the search grid (the scan is refused)
//   [74] what the deskew reports (leading points moved)   [75] = epoch when a device-wide scan gave up waiting
//   [76], [77] tile tickets of the two single-launch scans
//   [78], [79] queries of the neighbour search that start first (sparse neighbourhood) / after them
//   [80] workgroup ticket of the prologue (zero between launches: the workgroup that draws the last one clears it)
//   [81..94] developer counts: queries of the neighbour search that took each of its paths (kPath* below)
constexpr int kCounterWords = 96;
constexpr int kIndefiniteCounter = 72;
constexpr int kBeyondGrid = 73;
constexpr int kDeskewedCounter = 74;
constexpr int kScanTimeout = 75;
constexpr int kTicketA = 76;
constexpr int kTicketB = 77;
constexpr int kHeavyQueries = 78;
constexpr int kLightQueries = 79;
constexpr int kTicketP = 80;
// The paths of knn_search_kernel (vgicp_preprocess.hip): every query keeps a mask of the ones it took, and a context
// created with VGICP_DEBUG_PREP adds 1 to word kPathWord0 + bit for every bit set -- the number of queries that took
// the path (vgicp_prepare_search_report, include/vgicp_hip_search_report.h, in this order).
constexpr int kPathWord0 = 81;
constexpr int kPathCount = 14;
constexpr uint32_t kPathHome = 1u << 0;        // the query's own cell is its first candidates (has_home)
constexpr uint32_t kPathCrowded = 1u << 1;     // an own cell holds K points but more than kHomePoints
constexpr uint32_t kPathNoOwnCell = 1u << 2;   // no own cell on any level holds K points
constexpr uint32_t kPathWindowIsK = 1u << 3;   // the opening window holds exactly K entries: bound from their maximum
constexpr uint32_t kPathWholeScan = 1u << 4;   // no level's 27-cell block covers the ball: every point of the scan
constexpr uint32_t kPathClipped = 1u << 5;     // the 27-cell block reaches over the grid's edge
constexpr uint32_t kPathOpen2 = 1u << 6;       // a cell opened two levels down
constexpr uint32_t kPathOpen1 = 1u << 7;       // a level-1 cell opened one level down
constexpr uint32_t kPathLeaf = 1u << 8;        // a cell above the finest level measured
constexpr uint32_t kPathFinest = 1u << 9;      // a finest cell measured
constexpr uint32_t kPathCompacted = 1u << 10;  // the pool of waiting cells compacted
constexpr uint32_t kPathSpilled = 1u << 11;    // no room in the pool even so: the cell measured instead of opened
constexpr uint32_t kPathWaited = 1u << 12;     // candidates of a batch waited for room in the buffer
constexpr uint32_t kPathReranked = 1u << 13;   // more than 56 entries survived the select: all-pairs ranking
static_assert(kPathWord0 + kPathCount <= kCounterWords, "the path counts lie inside the counter block");
// the prologue finds the deskew's segments itself (no launch for the bounds) for ordered state queues up to this many
// states (8 bytes of LDS each) and sweeps up to this many workgroups of 256 points (a look-back slot each)
constexpr uint32_t kFusedBoundsStatesMax = 4096;
constexpr uint32_t kFusedBoundsBlocksMax = 4096;
constexpr uint32_t kDeskewMaxStates = 4096;   // the parallel deskew bounds keep 12 bytes per state in LDS; longer (or unordered) queues take the serial walk
constexpr uint32_t kPrepareMaxStates = 16000;  // IMU states that can own points of ONE sweep in the fused preparation (LDS)
constexpr uint32_t kMaxScanTiles = 4096;  // x 2 048 points: scans up to 8 M points
size_t preprocess_scratch_bytes(uint32_t n);
int preprocess_max_knn();
uint64_t preprocess_cell_entries(uint32_t cells);
size_t preprocess_cell_bytes(uint64_t entries);
size_t preprocess_tile_bytes();  // the tile slots of the two device-wide scans (allocated once per context, zeroed)
// CloudPreprocessor::process after the upload, enqueued as ONE sequence with no host round trip in it:
// [deskew bounds] -> extrinsic + deskew + Morton codes (+ clears) -> sort -> runs / kept points / query list ->
// output slots -> octree cells -> exact k-NN -> covariances.  Everything the host does not know yet (kept points,
// cells) stays on the device: tables and grids are sized from n.  pts: n x 3 on the device, moved in place by the
// extrinsic and the deskew.  Outputs: AoS points / covariances / indices (capacity n) and, when soa != nullptr, the
// 12 SoA planes the registration reads.  counters: the context's counter block (layout above); epoch: a number
// that differs from call to call (never 0).
struct PrepareArgs {
  double* pts;
  uint32_t n;
  double voxel_size;
  int knn;
  const double* extrinsic16;     // host, column-major 4x4, or nullptr
  const double* point_time;      // device, n (deskew) or nullptr
  const double* state_time;      // device, `states` timestamps
  const double* poses;           // device, 12 doubles per state
  uint32_t states;               // 0 = no deskew
  bool ordered_states;
  bool max_hits_known;           // max_hits below is set (the host has walked the capture times)
  uint32_t max_hits;             // the largest number of states whose timestamp is not above a point's capture time (all: a NaN time)
  uint32_t* ends;                // device scratch, deskew_scratch_words(states)
  void* scratch;                 // preprocess_scratch_bytes(n)
  void* cell_table;              // preprocess_cell_bytes(preprocess_cell_entries_for(n))
  uint64_t table_entries;
  double* out_pts;
  double* out_covs;
  unsigned long long* out_idx;
  double* soa;                   // optional
  uint64_t soa_stride;
  uint32_t* counters;
  unsigned long long* host_kept; // optional, page-locked host memory as the device addresses it: receives epoch << 32 | kept
                                 // points as soon as the down-sampling knows it (vgicp_scan_fetch_begin waits for that)
  void* tiles;                   // preprocess_tile_bytes()
  uint32_t epoch;
  int debug;
  hipEvent_t ev_after_prologue;  // optional: recorded behind the prologue (extrinsic + deskew + codes)
  // The raw points may still be ARRIVING in page-locked host memory (the frame chain's upload without copy commands, as
  // pack_arena_kernel does it for vgicp_align): src_points != nullptr = n x 24 bytes of staging memory that host threads
  // fill in units of src_unit points (a multiple of 256), publishing unit u by storing src_seq into src_flags[16 * u];
  // the prologue then reads its points from there (a unit's workgroups wait for its flag, at most src_spin polls; a
  // wait that runs out is reported like a scan's: counters[kScanTimeout] = epoch) and writes them to `pts`.
  // src_flags == nullptr with src_points set: everything is staged already.
  const char* src_points;
  const uint32_t* src_flags;
  uint32_t src_seq, src_unit, src_spin;
  // src_step != 0: the staging memory holds the sensor's own records (a PointCloud2 payload, vgicp_sweep_stage_cloud2):
  // src_step bytes per point (a multiple of 4, at most 64), float32 x, y, z at byte offsets src_off[0..2]; the prologue
  // widens them (float -> double is exact).  src_step == 0: n x 3 doubles.
  uint32_t src_step, src_off[3];
};
// The prepared scan (AoS on the device: kept x 3 doubles, kept x 9 doubles; kept and the refusal flags read from the
// counter block) written by a KERNEL into page-locked host memory in pieces of piece_bytes, every piece published by
// storing seq into flags[16 * piece] — the download of vgicp_scan_fetch_end, the mirror image of pack_arena_kernel.
// Layout of `stage`: the points, padded to a multiple of 256 bytes, then the covariances.  hdr_done receives
// seq << 32 | 1 (refused / nothing prepared) or seq << 32 first thing.  sums (device, 65 words, zero on entry and on
// exit) / host_sums (page-locked, 64 words): position-weighted word sums of what was copied, see fetch_kernel.
hipError_t launch_fetch(hipStream_t s, const double* aos_pts, const double* aos_cov, const uint32_t* counters, uint32_t epoch,
                        uint32_t n_cap, char* stage, uint32_t* flags, unsigned long long* hdr_done, uint32_t seq,
                        uint32_t piece_bytes, unsigned long long* sums, unsigned long long* host_sums);
hipError_t launch_prepare(hipStream_t s, const PrepareArgs& a);        // = head + tail
// head: the kernels that read the raw sweep (deskew bounds from the times, prologue); tail: everything behind them.
// A host that stages the sweep itself launches the head, finishes staging and launches the tail, so that the device
// reads the first units while the later ones are still being copied.
hipError_t launch_prepare_head(hipStream_t s, const PrepareArgs& a);
hipError_t launch_prepare_tail(hipStream_t s, const PrepareArgs& a);
// true: the head finds the deskew's segments inside the prologue (PrepareArgs::max_hits must be known), and a workgroup
// reads the capture times of ITS points only, behind the wait for their unit: a host that stages the sweep itself may
// then stage the times unit by unit with the points instead of before the launch
bool prepare_bounds_fused(uint32_t n, uint32_t states, bool ordered_states);
uint64_t preprocess_cell_entries_for(uint32_t n);  // from the number of points alone (no host round trip)
// The library's sort (vgicp_sort.h) of n (64-bit key, index) pairs for callers outside vgicp_preprocess.hip, where its
// 64-bit instantiation lives: (keys_a, idx_a) hold the input and are overwritten, the result is left in (keys_b, idx_b);
// split: sort_keys64_scratch_bytes(n) bytes.  Keys lie below ~0.  *launches (may be nullptr): kernels enqueued.
size_t sort_keys64_scratch_bytes(uint32_t n);
hipError_t launch_sort_keys64(hipStream_t s, unsigned long long* keys_a, uint32_t* idx_a, unsigned long long* keys_b,
                              uint32_t* idx_b, void* split, uint32_t n, uint32_t* launches);
// kernels enqueued by the launchers of this module since the counter was last reset (per host thread)
extern thread_local uint64_t g_kernel_launches;
#ifdef __HIPCC__   // a host compiler that only reads the layouts (tests/native) has no launch syntax
// How every launcher of the module enqueues a kernel: counted and launched in one statement (always inlined: no call
// stands between a launcher and its launch, and the module exports no instantiation).  A launcher reads hipGetLastError()
// once, at its end.  The sort adds launches_for(n) for its own launches: vgicp_sort.h is also built without the module.
template <typename Kernel, typename... Args>
static inline __attribute__((always_inline)) void counted_launch(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes,
                                                                hipStream_t s, const Args&... args) {
  ++g_kernel_launches;
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
}
#endif
// workgroups of `block` threads that cover `work` items
inline uint32_t blocks_for(uint64_t work, uint32_t block) { return (uint32_t)((work + block - 1) / block); }
hipError_t launch_transform_points(hipStream_t s, double* pts, uint32_t n, const double T16[16]);
// CloudPreprocessor::deskew: ends = scratch of deskew_scratch_words(states) words (the first `states` are the
// segment ends); poses = 12 doubles per state (R column-major, t); ordered_states: the host has checked that the
// state times are finite and non-decreasing (the parallel bounds; otherwise the reference's walk, state by state)
size_t deskew_scratch_words(uint32_t states);
hipError_t launch_deskew(hipStream_t s, double* pts, uint32_t n, const double* point_time, const double* state_time,
                         uint32_t states, const double* poses, uint32_t* ends, bool ordered_states);
// The raw points of the map (VGICP_OPTION_MAP_RAW_POINTS; LocalMap's Voxel::points, include/ESKF_LIO/LocalMap.hpp:63-87):
// an append log of every point an insertion ACCEPTED (the constructor, or addPoint while count < max), as prepare_point
// transformed it.  slot: the voxel's table slot (its identity: a tombstone is never claimed again, so the entries of an
// evicted voxel are dead and stay dead); ordinal: the voxel's count before the point, i.e. its index in Voxel::points.
struct RawPoint {
  double xyz[3];
  uint32_t slot;
  uint32_t ordinal;
};
static_assert(sizeof(RawPoint) == 32, "one raw point = 32 bytes");
// ctr[0] entries appended so far, ctr[1] != 0 when an append did not fit (nothing is written then), ctr[2] scratch of
// the compaction.  entries == nullptr: the store is off.
struct RawLog {
  RawPoint* entries = nullptr;
  uint32_t capacity = 0;
  uint32_t* ctr = nullptr;
};
// keep (launch_map_insert): one byte per point, 0 = the point is not inserted (a gated insertion refused it: no probe, no
// claim, not counted as lost), or nullptr: every point is.
hipError_t launch_map_insert(hipStream_t s, VoxelRecord* table, uint32_t mask, double voxel_size,
                             const double* points_aos, const double* covs_aos, uint32_t n,
                             const double pose12[12], uint64_t max_points, void* scratch,
                             size_t scratch_bytes, uint32_t* counters, bool short_lists = false,
                             const RawLog& raw = RawLog(), const uint8_t* keep = nullptr);
// The log's live entries (slot FULL in `table`; with `claimed`, the rehash's old-slot -> new-slot words, those whose
// old slot was carried over, renamed to the new slot) appended to dst; ctr[2] (zero before) counts them.  The source
// holds *ctr[0] entries, at most `src_upper`; `slots`: of `table` (or of the old table that `claimed` covers).
hipError_t launch_raw_compact(hipStream_t s, const RawPoint* src, uint32_t src_upper, const uint32_t* ctr,
                              const VoxelRecord* table, uint64_t slots, const uint32_t* claimed, RawPoint* dst,
                              uint32_t dst_capacity, uint32_t* dst_ctr);
// Output offsets of the export: offsets[slot] = where the voxel's points start (FULL slots, unspecified voxel order,
// each voxel's `count` points contiguous); *total (zero before) = the sum of count.  offsets may be nullptr (size only).
hipError_t launch_raw_offsets(hipStream_t s, const VoxelRecord* table, uint64_t slots, uint32_t* offsets, uint32_t* total);
// Every live entry to keys / points[offsets[slot] + ordinal] (positions at or beyond `capacity` are dropped).
hipError_t launch_raw_scatter(hipStream_t s, const RawPoint* log, uint32_t upper, const uint32_t* ctr,
                              const VoxelRecord* table, uint64_t slots, const uint32_t* offsets, uint32_t capacity,
                              int32_t* keys, double* points);
// short_lists: no sort — every voxel's points hang on a list (the record's spare word) that the voxel's first point
// walks in scan order.  For scans that put a handful of points into a voxel at most (a scan the device down-sampled
// itself); correct for any scan, quadratic in the points of one voxel beyond eight.
// Erase every voxel whose centre is farther than `distance` from `position`; counters[0] += erased.
hipError_t launch_map_evict(hipStream_t s, VoxelRecord* table, uint64_t slots, double voxel_size,
                            const double position[3], double distance, uint32_t* counters);
// Free-space carving (include/vgicp_hip_map_carve.h has the rule): two launches.  MARK, one lane per point of the scan
// (AoS, as the insertion reads it): the shield lookup, and the point's ray through the table if it casts one; hits and the
// shield bit go into the LOW half of the record's spare word (kCarveShield | hits: the insertion's list head, zero
// between insertions; the upper half is the dense copy's index and is left alone).  SWEEP, one lane per slot: decide,
// write SLOT_TOMB, put the low half back to 0.  Any of the counter pointers may be nullptr; every word only grows.
constexpr uint32_t kCarveShield = 0x80000000u;
struct CarveArgs {
  VoxelRecord* table;
  uint64_t slots;              // a power of two
  double voxel_size;
  const double* points_aos;    // n x 3
  uint32_t n;
  uint32_t stride, min_hits;
  double pose[12];             // R column-major (9), t (3)
  double origin[3], margin, max_range;
  uint32_t* rays;              // mark
  unsigned long long* visits;  // mark
  uint32_t* touched;           // sweep: FULL voxels with >= 1 hit
  uint32_t* shielded;          // sweep: ... of which shielded
  uint32_t* removed;           // sweep; also the length of keys
  int32_t* keys;               // sweep: the removed voxels' keys, 3 each, or nullptr
  uint32_t keys_capacity;      // voxels
};
hipError_t launch_map_carve(hipStream_t s, const CarveArgs& args);
// The ray report (include/vgicp_hip_map_rays.h has the rule): two launches per group of poses, each one lane per point
// and pose (grid.y = the group's poses).  CONFIRM: the lookup of the point's own voxel, whose slot's bit goes into the
// pose's bitmap (zero before).  WALK: the point's ray through the table up to the first FULL voxel, its class from the
// bitmap, the planes (single pose) and the counts.  The table is only read.
constexpr uint32_t kRayCountWords = 10;   // per pose, 64-bit: rays, visits, by_class[8] (vgicp_ray_counts)
struct RayArgs {
  const VoxelRecord* table;
  uint64_t slots;              // a power of two
  double voxel_size;
  const double* points_aos;    // n x 3
  uint32_t n, stride;
  const double* poses;         // device: 12 per pose of the group (R column-major, t)
  uint32_t n_poses;            // of the group
  double origin[3], margin, beyond, max_range;
  uint32_t* bits;              // slots / 32 words per pose of the group
  unsigned long long* counts;  // kRayCountWords per pose of the group; every word only grows
  uint8_t* status;             // the planes: nullptr, or n entries (n_poses == 1)
  double* range;
  int32_t* hit_key;
  uint32_t* steps;
};
hipError_t launch_map_rays(hipStream_t s, const RayArgs& args);
// Submap as scan (include/vgicp_hip_map_submap.h has the rule): three launches over the source table in groups of
// kSubmapGroupSlots slots (vgicp_submap_plan.h).  MARK decides per slot and leaves a ballot per 64 slots and three
// counts per group; SCAN (one workgroup) turns the groups' selected counts into exclusive offsets and writes the totals
// {selected, too far, too few} to `totals` and to totals_host (page-locked memory); EMIT writes the selected voxels,
// transformed, at their ranks: both layouts of a resident scan, the keys and the counts.  The table is only read.
struct SubmapArgs {
  const VoxelRecord* table;
  uint64_t slots;
  double voxel_size;             // of the source table
  double center[3], radius;
  uint64_t min_count;
  double pose[12];               // the frame: R column-major (9), t (3)
  unsigned long long* ballots;   // kSubmapGroupWords per group
  uint32_t* group_counts;        // [3][groups]: selected (after SCAN: the exclusive offsets), too far, too few
  uint32_t groups;
  uint32_t capacity;             // points the outputs hold: ranks at or beyond it are dropped
  unsigned long long* totals;    // 3 words
  double* aos_points;            // capacity x 3
  double* aos_covs;              // capacity x 9
  double* planes;                // kScanPlanes planes of `stride` doubles
  uint64_t stride;
  int32_t* keys;                 // capacity x 3
  unsigned long long* counts;    // capacity
};
hipError_t launch_submap(hipStream_t s, const SubmapArgs& args, unsigned long long* totals_host);
// Map merge (include/vgicp_hip_map_merge.h has the rule): the submap's MARK and SCAN over the source table as they are
// (sub: its selection, frame, ballots, group counts and totals; sub.capacity = n), then MOVE-AND-CLAIM (a selected lane
// transforms its record, finds or claims the slot in `table` and writes moved[rank], slot_in[rank], idx_in[rank] = rank;
// ranks from the selected total up to n get kNoSlot), the library's stable sort of (slot, rank) and APPLY (the head of a
// segment folds its contributors in rank order and writes the record once).  counters[0] += voxels created, counters[1]
// += contributors that found the table full; totals (64-bit, kMergeTotalWords, zero before): [4] += voxels updated,
// [5] += contributors frozen out, [6] += points accepted.  The source table is only read.
struct MergeMoved;   // vgicp_merge_plan.h
struct MergeArgs {
  SubmapArgs sub;
  VoxelRecord* table;            // the destination's
  uint32_t mask;                 // its slots - 1
  uint32_t n;                    // contributors the scratch holds: the source's voxel count as the host knows it
  double voxel_size;             // the destination's
  uint64_t max_count;            // 0: no cap
  MergeMoved* moved;             // n
  uint32_t* slot_in;             // n each; the sort leaves its result in (slot_out, idx_out)
  uint32_t* idx_in;
  uint32_t* slot_out;
  uint32_t* idx_out;
  void* split;                   // merge_sort_split_bytes(n)
  uint32_t* counters;
  unsigned long long* totals;
};
hipError_t launch_map_merge(hipStream_t s, const MergeArgs& args, unsigned long long* totals_host);
// Map checkpoint (include/vgicp_hip_map_checkpoint.h has the format): the submap's three launches over the same groups,
// with two ballots per 64 slots (FULL, TOMB).  MARK leaves the ballots, per ballot word the sum of its FULL records'
// counts (word_raw, raw points only) and three counts per group; SCAN (one workgroup) turns the groups' counts into
// exclusive offsets and writes the totals {FULL, TOMB, raw points} to `totals` and to totals_host (page-locked memory);
// EMIT writes the ascending slot lists, the records at their ranks (eight lanes per record; the spare word as zero) and
// per FULL slot the offset of its points in the raw section.  The table is only read.
struct CheckpointArgs {
  const VoxelRecord* table;
  uint64_t slots;
  unsigned long long* ballots;   // [groups][2][kSubmapGroupWords]
  uint32_t* word_raw;            // [groups][kSubmapGroupWords], or nullptr: no raw points
  uint32_t* group_counts;        // [3][groups]: FULL, TOMB, raw (after SCAN: the exclusive offsets)
  uint32_t groups;
  uint32_t full_capacity, tomb_capacity;   // entries the lists (and `records`) hold: ranks at or beyond are dropped
  unsigned long long* totals;    // 4 words
  uint32_t* full_slots;
  uint32_t* tomb_slots;
  VoxelRecord* records;
  uint32_t* offsets;             // [slots], written at FULL slots; or nullptr
};
hipError_t launch_checkpoint(hipStream_t s, const CheckpointArgs& args, unsigned long long* totals_host);
// ... and every live entry of the log to points[offsets[slot] + ordinal] (3 doubles; positions at or beyond `capacity`
// are dropped)
hipError_t launch_checkpoint_raw(hipStream_t s, const RawPoint* log, uint32_t upper, const uint32_t* ctr, const VoxelRecord* table,
                                 uint64_t slots, const uint32_t* offsets, uint32_t capacity, double* points);
// The restore: records[j] to table[full_slots[j]] (eight lanes per record), the state of table[tomb_slots[j]] to
// SLOT_TOMB; with raw points (log != nullptr) three more launches rebuild the log in canonical order — the sums of the
// counts per block of 1 024 records, their exclusive prefix sum, and the entries {xyz, full_slots[j], o} at offset[j] + o,
// ctr[0] = raw_points.  A slot at or beyond `slots` and a position at or beyond raw_points are dropped.  The table was
// cleared on the same stream.
struct RestoreArgs {
  VoxelRecord* table;
  uint64_t slots;
  const uint32_t* full_slots;
  const uint32_t* tomb_slots;
  const VoxelRecord* records;
  uint32_t voxels, tombstones;
  const double* raw;             // raw_points x 3
  uint32_t raw_points;
  RawPoint* log;                 // or nullptr
  uint32_t log_capacity;
  uint32_t* ctr;                 // RawLog::ctr
  uint32_t* block_sums;          // one word per 1 024 records
  unsigned long long* totals;    // 4 words
};
hipError_t launch_restore(hipStream_t s, const RestoreArgs& args);
// Append every FULL record to the output arrays (unordered); counters[0] = records written.
hipError_t launch_map_export(hipStream_t s, const VoxelRecord* table, uint64_t slots, uint32_t capacity,
                             int32_t* keys, double* means, double* covs, uint64_t* counts,
                             uint32_t* counters);

}  // namespace vgicp
