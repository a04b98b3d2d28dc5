// vgicp_kernels.hip — hand-written CDNA4 (gfx950) kernels of the VGICP registration path.
//
// Reference behaviour each kernel reproduces (paths relative to the reference checkout):
//   iterate_kernel  one round of the loop in ICP::align (src/Registration.cpp:15-28). Prologue: the
//                   merge of the previous round's partial sums, the LDLT solve, se3ToSE3, pose
//                   composition and convergence test (:71-79, :20-25, :37-50). Body:
//                   Open3D PointCloud::Transform of point + covariance (call sites :13,27),
//                   LocalMap::getVoxelIndex + voxelGrid_.find (src/LocalMap.cpp:94-100,114-118),
//                   ICP::computeJTJAndJTr (src/Registration.cpp:83-102) and the accumulation of
//                   ICP::computeTransform (:60-70)
//   evaluate_kernel that round's body at several given poses at once, plus the objective and the squared error
//                   (no counterpart in the reference: what Open3D's EvaluateRegistration is to its ICP)
// The voxel table's own kernels (clear, upsert, rehash, erase, match, dense copy) are vgicp_table.hip.
//
// Design notes (DESIGN.md has the numbers):
//   * The scan is never written back: the TOTAL pose is applied to the original point in registers
//     each round (the reference transforms a copy incrementally), so a point costs 96 B of reads.
//   * MFMA is not used: this is a gather plus a 27-value reduction at ~2 fp64 flop per byte.
//   * Reduction: 32-slot halving butterfly inside a 64-lane wave (32 exchanges instead of 6 x 28),
//     LDS across the waves of a workgroup, one plain 256-byte partial row per workgroup.  Nothing in a
//     launch waits for another workgroup: the NEXT launch's prologue folds the rows (every workgroup,
//     redundantly, in one fixed order — bit-reproducible) while its own scan loads are in flight, so
//     the kernel boundary is the only grid-wide synchronisation and no workgroup runs a serial tail
//     alone (the first version's ticket + write-through + last-workgroup tail cost 13 us per round).
#include <array>
#include <utility>

#include "vgicp_device.h"
#include "vgicp_device_fn.h"
#include "vgicp_launch_plan.h"
#include "vgicp_points_plan.h"

namespace vgicp {
namespace {

// Every covariance of the resident scan is bitwise symmetric (nine planes are read instead of twelve): the word that
// pack_scan_kernel sets to the scan's sequence number when one is not still differs from it.  nullptr = unknown, read all.
template <typename Args>
__device__ __forceinline__ bool scan_cov_symmetric(const Args& a) {
  return a.asym_dev != nullptr && *a.asym_dev != a.scan_seq;
}

// The 96-byte payload {mean, covariance} as six 16-byte pieces that lie PIECES double2 apart: 1 in a record, the number
// of worker threads in the plane-major neighbour-prefetch area of the persistent launch's LDS.
template <int PIECES = 1>
__device__ __forceinline__ void unpack_payload(const double2* pay, double (&mu)[3], double (&S)[9]) {
  const double2 a0 = pay[0 * PIECES], a1 = pay[1 * PIECES], a2 = pay[2 * PIECES],
                a3 = pay[3 * PIECES], a4 = pay[4 * PIECES], a5 = pay[5 * PIECES];
  mu[0] = a0.x; mu[1] = a0.y; mu[2] = a1.x;
  S[0] = a1.y; S[1] = a2.x; S[2] = a2.y; S[3] = a3.x; S[4] = a3.y; S[5] = a4.x;
  S[6] = a4.y; S[7] = a5.x; S[8] = a5.y;
}
// Payload of a record whose slot is known (an unchanged key that hit last round): one round trip.
__device__ __forceinline__ void load_payload(const VoxelRecord* rec, double (&mu)[3], double (&S)[9]) {
  unpack_payload(reinterpret_cast<const double2*>(rec->mean), mu, S);  // 16-byte aligned
}
// Lookup + payload: probe the key word(s), then fetch the 96-byte payload of the matching record as
// six 16-byte loads (same 128-byte line as the key, so they are L1/L2 hits).  Requesting key and
// payload together was measured slower: every lane addresses its own line, so each extra wave-level
// load costs 64 tag lookups whether or not the lane ends up matching.
__device__ __forceinline__ bool find_and_load(const VoxelRecord* table, uint32_t mask, int32_t kx,
                                              int32_t ky, int32_t kz, double (&mu)[3],
                                              double (&S)[9]) {
  const VoxelRecord* rec = find_voxel(table, mask, kx, ky, kz);
  if (rec == nullptr) return false;
  load_payload(rec, mu, S);
  return true;
}

// Value of lane ^ MASK for MASK in {8, 4, 2, 1}, by DPP inside the 16-lane row (VALU moves; ds_bpermute
// would send each value through the LDS crossbar and put its latency on the reduction's dependent path):
// 8 = rotate the row by 8; 4 = shift by 4 towards the lower lanes for banks 0 and 2, towards the upper ones
// for banks 1 and 3; 2 and 1 = quad permutes.
template <int MASK>
__device__ __forceinline__ int xor_lane_i32(int x) {
  static_assert(MASK == 8 || MASK == 4 || MASK == 2 || MASK == 1, "row-local masks only");
  if constexpr (MASK == 8) return __builtin_amdgcn_update_dpp(x, x, 0x128 /* row_ror:8 */, 0xF, 0xF, false);
  if constexpr (MASK == 4) {
    const int lower = __builtin_amdgcn_update_dpp(x, x, 0x104 /* row_shl:4 */, 0xF, 0x5, false);
    return __builtin_amdgcn_update_dpp(lower, x, 0x114 /* row_shr:4 */, 0xF, 0xA, false);
  }
  if constexpr (MASK == 2) return __builtin_amdgcn_update_dpp(x, x, 0x4E /* quad_perm:[2,3,0,1] */, 0xF, 0xF, false);
  return __builtin_amdgcn_update_dpp(x, x, 0xB1 /* quad_perm:[1,0,3,2] */, 0xF, 0xF, false);
}
template <int MASK>
__device__ __forceinline__ double xor_lane_f64(double v) {
  return __hiloint2double(xor_lane_i32<MASK>(__double2hiint(v)), xor_lane_i32<MASK>(__double2loint(v)));
}

// One halving step of the wave butterfly: N live values -> N/2, exchanging with lane ^ MASK.
template <int N, int MASK>
__device__ __forceinline__ void fold(double (&v)[kSlots], bool upper) {
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    const double keep = upper ? v[j + N / 2] : v[j];
    const double send = upper ? v[j] : v[j + N / 2];
    v[j] = keep + xor_lane_f64<MASK>(send);
  }
}

// The two widest halving steps without LDS and without selects: v_permlane32_swap / v_permlane16_swap
// (gfx950) exchange the upper half (odd 16-lane rows) of one register with the lower half (even rows)
// of another, which is exactly "keep my half of the slots, receive the partner's": 3 instructions per
// pair of slots instead of 7.
template <int N, bool ROW16>
__device__ __forceinline__ void fold_swap(double (&v)[kSlots]) {
#pragma unroll
  for (int j = 0; j < N / 2; ++j) {
    const unsigned alo = (unsigned)__double2loint(v[j]), ahi = (unsigned)__double2hiint(v[j]);
    const unsigned blo = (unsigned)__double2loint(v[j + N / 2]), bhi = (unsigned)__double2hiint(v[j + N / 2]);
    const auto lo = ROW16 ? __builtin_amdgcn_permlane16_swap(alo, blo, false, false)
                          : __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    const auto hi = ROW16 ? __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false)
                          : __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    v[j] = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
  }
}

// The wave's part of a round's reduction: the 32-slot halving butterfly, after which lane l holds slot (l >> 1) summed
// over the 64 lanes, handed to the workgroup through the wave's row of LDS.
__device__ __forceinline__ void wave_fold_to_lds(double (&v)[kSlots], uint32_t lane, double* red_row) {
  fold_swap<32, false>(v);
  fold_swap<16, true>(v);
  fold<8, 8>(v, (lane & 8) != 0);
  fold<4, 4>(v, (lane & 4) != 0);
  fold<2, 2>(v, (lane & 2) != 0);
  const double wsum = v[0] + xor_lane_f64<1>(v[0]);
  if ((lane & 1) == 0) red_row[lane >> 1] = wsum;
}

// 1 / d for a normal, finite d by v_rcp_f64 (good to 2^-24) + ONE third-order step y (1 + e + e^2), e = 1 - d y: three
// dependent FMAs, error 2^-72 before the last rounding — the correctly rounded quotient for all of 4 M random
// arguments (tools/micro/rcp_accuracy.hip), as the two Newton steps of rounds 1-4 were, with one instruction less on
// the chain; a quarter of the dependent instructions of the IEEE division.
__device__ __forceinline__ double rcp_newton(double d) {
  const double y = __builtin_amdgcn_rcp(d);
  const double e = fma(-d, y, 1.0);
  return fma(y, fma(e, e, e), y);
}

// Fallback of the 6x6 solve: vgicp_math.h's ldlt6_solve — Eigen's pivoted LDLT with pseudo-inverted D, the
// operation order of the published algorithm, no contraction — run by lane 0 on an LDS work array (the
// pivoting makes every index dynamic), the solution then read by every lane.  It is taken only when the
// natural-order factorisation below meets a pivot that is not safely positive (singular or indefinite
// normal equations, "no correspondences" included), so its ~10 us of dependent LDS traffic are off the
// hot path.  packed: LDS, 21 lower-triangle entries then the 6 of J^T r; work: LDS, kSolveWork doubles.
// All 64 lanes of the wave must call it.
constexpr int kSolveWork = kLdltWork + 16;
__device__ __forceinline__ void ldlt6_solve_pivoted(const double* packed, double* work, uint32_t lane,
                                                    double (&x)[6]) {
  double* rhs = work + kLdltWork;
  double* sol = work + kLdltWork + 8;
  if (lane == 0) {
    for (int k = 0; k < 6; ++k) rhs[k] = -packed[21 + k];
    ldlt6_solve(packed, rhs, sol, work);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int k = 0; k < 6; ++k) x[k] = sol[k];
}

// sin and cos of a SMALL angle (|a| <= 0.5 rad; Gauss-Newton steps are far smaller) by their Taylor series in
// Horner form: truncation below 5e-17 relative, no argument reduction, ~20 dependent FMAs instead of the
// library's ~100 instructions.  Larger angles take the library call.
__device__ __forceinline__ void sincos_step(double a, double* s, double* c) {
  if (fabs(a) > 0.5) {  // uniform on the solver wave
    sincos(a, s, c);
    return;
  }
  const double z = a * a;
  double ps = -1.0 / 1307674368000.0;   // -1/15!
  ps = fma(ps, z, 1.0 / 6227020800.0);  //  1/13!
  ps = fma(ps, z, -1.0 / 39916800.0);   // -1/11!
  ps = fma(ps, z, 1.0 / 362880.0);      //  1/9!
  ps = fma(ps, z, -1.0 / 5040.0);       // -1/7!
  ps = fma(ps, z, 1.0 / 120.0);         //  1/5!
  ps = fma(ps, z, -1.0 / 6.0);          // -1/3!
  *s = fma(a * z, ps, a);
  double pc = 1.0 / 20922789888000.0;   //  1/16!
  pc = fma(pc, z, -1.0 / 87178291200.0);  // -1/14!
  pc = fma(pc, z, 1.0 / 479001600.0);   //  1/12!
  pc = fma(pc, z, -1.0 / 3628800.0);    // -1/10!
  pc = fma(pc, z, 1.0 / 40320.0);       //  1/8!
  pc = fma(pc, z, -1.0 / 720.0);        // -1/6!
  pc = fma(pc, z, 1.0 / 24.0);          //  1/4!
  pc = fma(pc, z, -0.5);                // -1/2!
  *c = fma(pc, z, 1.0);
}

// Fast path of the 6x6 solve: LDL^T in natural order, fully unrolled, everything in registers with
// static indices (about 130 fp64 operations and 6 reciprocals; every lane of the wave runs the same
// scalar program).  For a symmetric positive definite system any elimination order is backward
// stable, so x differs from the pivoted solve only by rounding (~cond * 1e-16).  Returns false when a
// pivot is not safely positive — singular or indefinite normal equations, the all-zero system of
// "no correspondences" included — and the caller then runs the pivoted, Eigen-faithful solve above.
// A: 21 lower-triangle entries row by row; g: right-hand side (already negated J^T r).
__device__ __forceinline__ bool ldlt6_solve_spd(const double (&A)[21], const double (&g)[6],
                                                double (&x)[6]) {
  double L[6][6], W[6][6], inv[6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[tri6(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * W[j][k];
    ok = ok && (d > 1e-13 * A[tri6(j, j)]) && (d < 1.0e300) && (d > 1.0e-290);  // also false for NaN
    inv[j] = rcp_newton(d);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[tri6(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i][k] * W[j][k];
      W[i][j] = t;           // L(i,j) * D(j)
      L[i][j] = t * inv[j];
    }
  }
  double z[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double t = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[i][k] * z[k];
    z[i] = t;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double t = z[i] * inv[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= L[k][i] * x[k];
    x[i] = t;
  }
  return ok;
}

// se(3) exponential as vgicp_math.h's se3_exp (reference src/Utils.cpp:28-32,40-63) with the sine
// and cosine of the one angle taken from a single sincos call.
__device__ __forceinline__ void se3_exp_angle(const double* xi, Pose& T) {
  const double* r = xi + 3;
  const double n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  const double angle = sqrt(n2);
  double s, c;
  sincos_step(angle, &s, &c);
  double k[3] = {r[0], r[1], r[2]};
  const double inv_angle = (n2 > 1.0e-280) ? rcp_newton(angle) : 1.0 / angle;
  if (n2 > 0.0) { k[0] = r[0] * inv_angle; k[1] = r[1] * inv_angle; k[2] = r[2] * inv_angle; }
  const double sx = s * k[0], sy = s * k[1], sz = s * k[2];
  const double cx = (1.0 - c) * k[0], cy = (1.0 - c) * k[1], cz = (1.0 - c) * k[2];
  double tmp;
  tmp = cx * k[1]; T.R[3] = tmp - sz; T.R[1] = tmp + sz;
  tmp = cx * k[2]; T.R[6] = tmp + sy; T.R[2] = tmp - sy;
  tmp = cy * k[2]; T.R[7] = tmp - sx; T.R[5] = tmp + sx;
  T.R[0] = cx * k[0] + c;
  T.R[4] = cy * k[1] + c;
  T.R[8] = cz * k[2] + c;
  if (angle < 1e-6) {
    T.t[0] = xi[0]; T.t[1] = xi[1]; T.t[2] = xi[2];
    return;
  }
  const double f1 = s * inv_angle, f2 = (1.0 - c) * inv_angle;
  double J[9];
#pragma unroll
  for (int cc = 0; cc < 3; ++cc)
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) J[rr + 3 * cc] = (1.0 - f1) * k[rr] * k[cc];
  J[0] += f1; J[4] += f1; J[8] += f1;
  J[3] += -f2 * k[2]; J[6] += f2 * k[1];
  J[1] += f2 * k[2];  J[7] += -f2 * k[0];
  J[2] += -f2 * k[1]; J[5] += f2 * k[0];
  mat3_vec(J, xi, T.t);
}

// The same map for the steps Gauss-Newton actually takes (|phi| <= 0.5 rad), written in phi itself instead of
// (angle, axis): with n2 = |phi|^2,
//   A = sin a / a = 1 - n2 C,   B = (1 - cos a) / a^2,   C = (a - sin a) / a^3      (power series in n2)
//   R = (1 - n2 B) I + B phi phi^T + A [phi]x              (= cos a I + (1 - cos a) k k^T + sin a [k]x, reference src/Utils.cpp:28-32)
//   t = A rho + C phi (phi . rho) + B (phi x rho)          (= J_l(phi) rho, reference src/Utils.cpp:40-54)
// No square root, no reciprocal, no normalisation and no sine / cosine on the round's serial chain: the two series in
// Estrin form are 4 dependent operations deep after n2 (the angle-axis form: sqrt ~10, Taylor sincos 10, rcp 5, products
// 4).  Truncation < 1e-17 relative at |phi| = 0.5; the results agree with the angle-axis form to rounding (~1e-16), not bit for bit.
// The reference's branch "angle < 1e-6 -> t = rho" is kept: kSmallAngle2 is the smallest double whose square root rounds
// to >= 1e-6 (tests/test_capi_cpu.py checks the constant against sqrt).
constexpr double kSmallAngle2 = 0x1.19799812dea10p-40;   // 9.999999999999998e-13
__device__ __forceinline__ void se3_exp_device(const double* xi, Pose& T) {
  const double px = xi[0], py = xi[1], pz = xi[2], rx = xi[3], ry = xi[4], rz = xi[5];
  const double n2 = rx * rx + ry * ry + rz * rz;
  if (n2 > 0.25) {  // uniform on the solver wave
    se3_exp_angle(xi, T);
    return;
  }
  const double z2 = n2 * n2, z4 = z2 * z2;
  // B = sum (-1)^k n2^k / (2k + 2)!,  C = sum (-1)^k n2^k / (2k + 3)!,  k = 0 .. 7
  const double b01 = fma(n2, -1.0 / 24.0, 0.5), b23 = fma(n2, -1.0 / 40320.0, 1.0 / 720.0);
  const double b45 = fma(n2, -1.0 / 479001600.0, 1.0 / 3628800.0), b67 = fma(n2, -1.0 / 20922789888000.0, 1.0 / 87178291200.0);
  const double c01 = fma(n2, -1.0 / 120.0, 1.0 / 6.0), c23 = fma(n2, -1.0 / 362880.0, 1.0 / 5040.0);
  const double c45 = fma(n2, -1.0 / 6227020800.0, 1.0 / 39916800.0), c67 = fma(n2, -1.0 / 355687428096000.0, 1.0 / 1307674368000.0);
  const double B = fma(z4, fma(z2, b67, b45), fma(z2, b23, b01));
  const double C = fma(z4, fma(z2, c67, c45), fma(z2, c23, c01));
  const double A = fma(-n2, C, 1.0), c = fma(-n2, B, 1.0);
  const double bx = B * rx, by = B * ry, bz = B * rz, ax = A * rx, ay = A * ry, az = A * rz;
  T.R[0] = fma(bx, rx, c); T.R[4] = fma(by, ry, c); T.R[8] = fma(bz, rz, c);
  T.R[3] = fma(bx, ry, -az); T.R[1] = fma(bx, ry, az);
  T.R[6] = fma(bx, rz, ay);  T.R[2] = fma(bx, rz, -ay);
  T.R[7] = fma(by, rz, -ax); T.R[5] = fma(by, rz, ax);
  if (n2 < kSmallAngle2) {
    T.t[0] = px; T.t[1] = py; T.t[2] = pz;
    return;
  }
  const double cd = C * (rx * px + ry * py + rz * pz);
  T.t[0] = fma(A, px, fma(cd, rx, B * (ry * pz - rz * py)));
  T.t[1] = fma(A, py, fma(cd, ry, B * (rz * px - rx * pz)));
  T.t[2] = fma(A, pz, fma(cd, rz, B * (rx * py - ry * px)));
}

// Fixed-shape pairwise sum of N values: (first half) + (second half), recursively.  The order every fold of the
// partial sums uses, in both loop variants (hence the same bits), instead of a left-to-right chain: a dependent
// fp64 add costs ~32 cycles on one wave (tools/micro/valu_chain.hip), so 16 values take 4 steps instead of 15.
template <int N>
__device__ __forceinline__ double tree_sum(const double* v) {
  if constexpr (N == 1) return v[0];
  else return tree_sum<N / 2>(v) + tree_sum<N - N / 2>(v + N / 2);
}

// A pose as 12 doubles in memory (global, LDS, kernel arguments): R column-major, then t.
__device__ __forceinline__ void load_pose(const double* src, Pose& T) {
#pragma unroll
  for (int k = 0; k < 9; ++k) T.R[k] = src[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) T.t[k] = src[9 + k];
}
__device__ __forceinline__ void store_pose(double* dst, const Pose& T) {
#pragma unroll
  for (int k = 0; k < 9; ++k) dst[k] = T.R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) dst[9 + k] = T.t[k];
}

// What every wave needs to run a round: the total pose, or the news that the loop has ended.
struct RoundHead {
  Pose total;
  bool stop;
};

// LDS a workgroup of BLOCK threads needs for the prologue.
template <int BLOCK>
struct PrologueShared {
  double fin[BLOCK / kSlots][kSlots];
  double totals[kSlots];
  double work[kSolveWork];
  double pose[12];
  int stop;
};

// The two halves of a round's prologue, run by EVERY workgroup (identical arithmetic on identical
// inputs, so every workgroup derives the same pose).  Reference: the merge, solve, compose and
// convergence test of src/Registration.cpp:71-79, :20-25.
//
// prologue_fold: issue every global load (previous rows, state) before the first wait, fold the rows
// in a fixed order into LDS, return the OLD pose.  prologue_solve (wave 0 only): finish the fold,
// pivoted LDLT, se(3) exponential, compose, convergence test; the new pose goes to LDS, and from
// workgroup 0 to the state / log the next launch and the host read.
template <int BLOCK>
__device__ __forceinline__ RoundHead prologue_fold(const IterArgs& a, PrologueShared<BLOCK>& sh,
                                                   int& it, int& max_it, double& cos_thr,
                                                   double& tsq_thr) {
  constexpr int kGroups = BLOCK / kSlots;
  constexpr int kBatch = 16;  // independent loads in flight per thread; the add order stays fixed
  const uint32_t tid = threadIdx.x;
  const AlignState* in = a.state_in;

  const uint32_t slot = tid & (kSlots - 1), group = tid / kSlots;
  double row[kBatch];
#pragma unroll
  for (int u = 0; u < kBatch; ++u) {
    const uint32_t b = group + u * kGroups;
    row[u] = b < a.prev_rows ? a.prev[(size_t)b * kSlots + slot] : 0.0;
  }
  RoundHead head;
  load_pose(in->pose, head.total);
  it = in->iteration;
  max_it = in->max_iteration;
  cos_thr = in->cosine_threshold;
  tsq_thr = in->translation_sq_threshold;
  head.stop = in->done != 0;
  if (head.stop || a.prev_rows == 0) {
    // nothing to fold: either the loop ended in an earlier launch, or this is the first round
    if (blockIdx.x == 0 && tid == 0) *a.state_out = *in;
    return head;
  }
  double s = tree_sum<kBatch>(row);  // rows group, group + kGroups, ...: the 16 rows a folder of the persistent launch adds
  for (uint32_t b0 = group + kBatch * kGroups; b0 < a.prev_rows; b0 += kGroups * kBatch) {
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint32_t b = b0 + u * kGroups;
      row[u] = b < a.prev_rows ? a.prev[(size_t)b * kSlots + slot] : 0.0;
    }
    s += tree_sum<kBatch>(row);
  }
  sh.fin[group][slot] = s;
  return head;
}

// The pose prior (include/vgicp_hip_prior.h): what the solver wave adds in front of the solve, one function for
// prologue_solve and the persistent launch's solver section.  T: the pose the round's sums were taken at; totals (LDS):
// the round's 27 data sums, which are NOT touched (they go to the log as they are).  Returns (LDS) the sums the round
// solves with: A + G^T L G in the 21 lower-triangle slots, b + G^T L d in the 6 behind them, d and G being the chart
// of vgicp_math.h's pose_prior_chart.  All 64 lanes of the wave call it; the lanes share the congruence instead of each
// running it as straight-line code:
//   every lane  d and G's lower right block (pose_prior_chart_blocks: uniform, ~150 operations); lane 0 puts d, G and L into LDS
//   lanes 0-35  one entry of L G each, lanes 36-41 one entry of L d each
//   lanes 0-20  one entry of the lower triangle of G^T (L G) each, lanes 21-26 one entry of G^T (L d) each
// with a fixed order of the six products of every entry, so that every workgroup and both launches get the same bits.
struct PriorShared {
  double G[36];      // column-major
  double LG[36];     // column-major
  double d[6], Ld[6];
  double info[21];
  double solve[kSlots];
};
template <typename Args>
__device__ __forceinline__ const double* prior_solve_totals(const Args& a, const Pose& T, const double* totals,
                                                            uint32_t lane) {
  __shared__ PriorShared ps;
  Pose T0;
  load_pose(a.prior.pose, T0);
  double d[6], M[9];
  pose_prior_chart_blocks(T0, T, d, M);
  // G = [I, -[t]x; 0, M]: the zeros from 36 lanes, what is not zero from lane 0 (the same wave: LDS is in order within
  // it), laid out by the function the host's chart uses
  if (lane < 36) ps.G[lane] = 0.0;
  if (lane == 0) {
    pose_prior_chart_nonzero(T.t, M, ps.G);
#pragma unroll
    for (int k = 0; k < 6; ++k) ps.d[k] = d[k];
  }
  if (lane < 21) ps.info[lane] = a.prior.info[lane];   // one entry per lane, read from the dispatch packet's memory
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < 42) {
    const bool mat = lane < 36;
    const uint32_t i = mat ? lane % 6u : lane - 36u, j = mat ? lane / 6u : 0u;   // entry (i, j) of L G, entry i of L d
    const double* col = mat ? ps.G + 6u * j : ps.d;
    double sum = 0.0;
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
      const uint32_t hi = i > k ? i : k, lo = i > k ? k : i;
      sum += ps.info[hi * (hi + 1u) / 2u + lo] * col[k];
    }
    if (mat) ps.LG[lane] = sum;
    else ps.Ld[i] = sum;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < kSlots) {
    double sum = totals[lane];
    if (lane < (uint32_t)kNormalEq) {
      const bool mat = lane < 21u;
      // lane = tri6(i, j): the row is the largest i with i (i + 1) / 2 <= lane
      const uint32_t i = !mat ? lane - 21u : lane >= 15u ? 5u : lane >= 10u ? 4u : lane >= 6u ? 3u : lane >= 3u ? 2u : lane >= 1u ? 1u : 0u;
      const uint32_t j = mat ? lane - i * (i + 1u) / 2u : 0u;
      const double* left = ps.G + 6u * i;                   // column i of G = row i of G^T
      const double* right = mat ? ps.LG + 6u * j : ps.Ld;
      double add = 0.0;
#pragma unroll
      for (uint32_t k = 0; k < 6; ++k) add += left[k] * right[k];
      sum += add;
    }
    ps.solve[lane] = sum;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return ps.solve;
}

// PRIOR: the round solves with the prior's terms on top of the data sums (prior_solve_totals); the log keeps the data sums.
template <int BLOCK, bool PRIOR = false>
__device__ __forceinline__ void prologue_solve(const IterArgs& a, PrologueShared<BLOCK>& sh,
                                               const Pose& old_total, uint32_t lane, int it,
                                               int max_it, double cos_thr, double tsq_thr) {
  constexpr int kGroups = BLOCK / kSlots;
  double tot = 0.0;
  if (lane < kSlots) {
    double part[kGroups];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) part[g] = sh.fin[g][lane];
    tot = tree_sum<kGroups>(part);
  }
  // the 27 sums to every lane (same wave wrote them: LDS is in order within a wave)
  if (lane < kSlots) sh.totals[lane] = tot;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const double* solve = sh.totals;
  if constexpr (PRIOR) solve = prior_solve_totals(a, old_total, sh.totals, lane);
  double A[21], g[6], xi[6];
#pragma unroll
  for (int k = 0; k < 21; ++k) A[k] = solve[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) g[k] = -solve[21 + k];
  if (!ldlt6_solve_spd(A, g, xi)) ldlt6_solve_pivoted(solve, sh.work, lane, xi);  // uniform branch
  Pose step, next;
  se3_exp_device(xi, step);
  pose_compose(step, old_total, next);
  const bool conv = converged(step, cos_thr, tsq_thr);
  const bool stop = conv || (it + 1 >= max_it);
  if (lane == 0) {
    store_pose(sh.pose, next);
    sh.stop = stop ? 1 : 0;
  }
  if (blockIdx.x == 0) {
    if (lane < kSlots) a.log[(size_t)it * kSlots + lane] = tot;
    if (lane == 0) {
      AlignState* out = a.state_out;
#pragma unroll
      for (int k = 0; k < 9; ++k) { out->pose[k] = next.R[k]; out->step[k] = step.R[k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) { out->pose[9 + k] = next.t[k]; out->step[9 + k] = step.t[k]; }
      out->cosine_threshold = cos_thr;
      out->translation_sq_threshold = tsq_thr;
      out->max_iteration = max_it;
      out->iteration = it + 1;
      out->converged = conv ? 1 : 0;
      out->done = stop ? 1 : 0;
    }
  }
}

__device__ __forceinline__ void load_point(const double* scan, uint64_t stride, uint32_t i,
                                           double (&q)[kScanPlanes]) {
  const double* s = scan + i;
#pragma unroll
  for (int k = 0; k < kScanPlanes; ++k) q[k] = s[k * stride];
}

// The same for a scan whose covariances are ALL bitwise symmetric (pack_scan_kernel found no exception): the three
// planes above the diagonal are copies of the three below it and are not read — 72 instead of 96 bytes per point.
__device__ __forceinline__ void load_point_sym(const double* scan, uint64_t stride, uint32_t i,
                                               double (&q)[kScanPlanes], bool symmetric) {
  if (!symmetric) {
    load_point(scan, stride, i, q);
    return;
  }
  const double* s = scan + i;
  // planes: x y z c00 c10 c20 c01 c11 c21 c02 c12 c22
  q[0] = s[0]; q[1] = s[stride]; q[2] = s[2 * stride];
  q[3] = s[3 * stride]; q[4] = s[4 * stride]; q[5] = s[5 * stride];
  q[7] = s[7 * stride]; q[8] = s[8 * stride]; q[11] = s[11 * stride];
  q[6] = q[4]; q[9] = q[5]; q[10] = q[8];
}

// One correspondence: p (already in the map frame), scan covariance C, voxel mean / covariance.
// ICP::computeJTJAndJTr in structured form (J = [I | -[p]x]); S holds C_voxel on entry.
template <bool B>
struct Flag { static constexpr bool value = B; };

// W = S^-1 by cofactors as Eigen's fixed-size inverse (vgicp_math.h inv3), the one division replaced by
// v_rcp_f64 + one third-order step (rcp_newton: ~1 ulp; a third of the dependent instructions)
__device__ __forceinline__ void inverse3_cofactor(const double (&S)[9], double (&W)[9]) {
  const double c00 = S[4] * S[8] - S[7] * S[5], c10 = S[5] * S[6] - S[8] * S[3], c20 = S[3] * S[7] - S[6] * S[4];
  const double det = c00 * S[0] + c10 * S[1] + c20 * S[2];
  const double id = rcp_newton(det);
  const double c01 = S[7] * S[2] - S[1] * S[8], c11 = S[8] * S[0] - S[2] * S[6], c21 = S[6] * S[1] - S[0] * S[7];
  const double c02 = S[1] * S[5] - S[4] * S[2], c12 = S[2] * S[3] - S[5] * S[0], c22 = S[0] * S[4] - S[3] * S[1];
  W[0] = c00 * id; W[3] = c10 * id; W[6] = c20 * id;
  W[1] = c01 * id; W[4] = c11 * id; W[7] = c21 * id;
  W[2] = c02 * id; W[5] = c12 * id; W[8] = c22 * id;
}

// The term of one correspondence, the ONE definition for the rounds (accumulate_match), the evaluation (evaluate_kernel)
// and the per-point report and gate (point_term): S = R C R^T + C_voxel (S holds C_voxel on entry), W = S^-1, and the
// raw squared Mahalanobis residual e^T W e for e = p - mu, formed as e . (W e).
__device__ __forceinline__ void match_weight(const double* R, const double (&C)[9], double (&S)[9], double (&W)[9]) {
  double RC[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      RC[r + 3 * c] = R[r] * C[3 * c] + R[r + 3] * C[1 + 3 * c] + R[r + 6] * C[2 + 3 * c];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r)
      S[r + 3 * c] += RC[r] * R[c] + RC[r + 3] * R[c + 3] + RC[r + 6] * R[c + 6];
  inverse3_cofactor(S, W);
}
__device__ __forceinline__ double mahalanobis(const double (&W)[9], double e0, double e1, double e2) {
  const double g0 = W[0] * e0 + W[3] * e1 + W[6] * e2;
  const double g1 = W[1] * e0 + W[4] * e1 + W[7] * e2;
  const double g2 = W[2] * e0 + W[5] * e1 + W[8] * e2;
  return e0 * g0 + e1 * g1 + e2 * g2;
}

// The robust round (include/vgicp_hip_robust.h): the settings as a kernel holds them, made once per launch from the
// three fields at the end of IterArgs / PersistArgs, and the weight of one correspondence from its squared Mahalanobis
// residual raw = e^T W e.  d^2 = max(raw, 0); the gate is asked of raw itself, so a NaN residual is rejected.  Huber:
// c / sqrt(d^2) = c^2 rsq(c^2 d^2), v_rsq_f64 + one third-order step y (1 + h/2 + 3 h^2/8), h = 1 - x y^2; Cauchy:
// c^2 / (c^2 + d^2) by rcp_newton.  Everything here but raw is uniform and stays in scalar registers: no lane takes a
// path of its own, a rejected correspondence has weight 0.
constexpr uint32_t kRobustHuber = 1, kRobustCauchy = 2;
struct RobustSetting {
  uint32_t kernel = 0;
  bool gated = false;
  double c2 = 1.0, gate = 0.0;
};
__device__ __forceinline__ RobustSetting robust_setting(uint32_t kernel, double scale2, double gate) {
  RobustSetting r;
  r.kernel = kernel;
  r.c2 = scale2;
  r.gated = gate > 0.0;
  r.gate = gate;
  return r;
}
__device__ __forceinline__ double robust_weight(const RobustSetting& r, double raw) {
  const double d2 = fmax(raw, 0.0);
  double w = 1.0;
  if (r.kernel == kRobustCauchy) {
    w = r.c2 * rcp_newton(r.c2 + d2);
  } else if (r.kernel == kRobustHuber) {
    const double x = r.c2 * d2;
    const double y = __builtin_amdgcn_rsq(x);
    const double h = fma(-x * y, y, 1.0);
    const double rs = fma(y * h, fma(h, 0.375, 0.5), y);
    w = d2 <= r.c2 ? 1.0 : r.c2 * rs;
  }
  const bool keep = !r.gated || raw <= r.gate;
  return keep ? w : 0.0;
}

// FIRST: v holds nothing yet (the thread's first match of the round): the 28 values are stored, not added to
// zeros — 28 dependent-latency adds less per round in the one-point-per-thread case.  Both loop variants make the
// same choice for the same point, so they still agree bit for bit.
// ROBUST: every one of the 27 sums takes the correspondence's weight as a factor (through W), the count takes (w > 0); a
// weight of exactly 1.0 leaves the plain bits.
template <bool FIRST, bool ROBUST = false>
__device__ __forceinline__ void accumulate_match(const double* R, const double (&p)[3],
                                                 const double (&C)[9], const double (&mu)[3],
                                                 double (&S)[9], double (&v)[kSlots],
                                                 const RobustSetting& robust = RobustSetting()) {
  double W[9];
  match_weight(R, C, S, W);
  auto acc = [](double& dst, double x) { if (FIRST) dst = x; else dst += x; };
  const double e0 = p[0] - mu[0], e1 = p[1] - mu[1], e2 = p[2] - mu[2];
  if constexpr (ROBUST) {
    // d^2 = e^T W e from W e, the weight from d^2; the count now, and W takes the weight as a factor BEFORE anything is
    // made of it: every one of the 27 sums below is linear in W, so each carries the factor w (nine products instead
    // of 27, and w is dead before Q is live).  w = 1.0 leaves W's bits.  A rejected correspondence (w = 0) gets W = +0
    // by SELECTION, not by the product: its W may be NaN (a non-finite covariance entry fails the gate), and NaN x 0
    // would put NaN into 27 sums of a round that does not count it.
    const double w = robust_weight(robust, mahalanobis(W, e0, e1, e2));
    const bool counted = w > 0.0;
    acc(v[kCountSlot], counted ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k] = counted ? W[k] * w : 0.0;
  }
  // Q = [p]x W  (rows 3..5, columns 0..2 of J^T Sigma^-1 J)
  double Q[9];  // Q[r + 3c]
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    Q[0 + 3 * c] = p[1] * W[2 + 3 * c] - p[2] * W[1 + 3 * c];
    Q[1 + 3 * c] = p[2] * W[0 + 3 * c] - p[0] * W[2 + 3 * c];
    Q[2 + 3 * c] = p[0] * W[1 + 3 * c] - p[1] * W[0 + 3 * c];
  }
  // lower triangle of J^T Sigma^-1 J, row by row
  acc(v[0], W[0]);
  acc(v[1], W[1]); acc(v[2], W[4]);
  acc(v[3], W[2]); acc(v[4], W[5]); acc(v[5], W[8]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int base = (3 + r) * (4 + r) / 2;
    const double q0 = Q[r], q1 = Q[r + 3], q2 = Q[r + 6];
    acc(v[base + 0], q0); acc(v[base + 1], q1); acc(v[base + 2], q2);
    acc(v[base + 3], q2 * p[1] - q1 * p[2]);
    if (r >= 1) acc(v[base + 4], q0 * p[2] - q2 * p[0]);
    if (r >= 2) acc(v[base + 5], q1 * p[0] - q0 * p[1]);
  }
  // J^T Sigma^-1 r
  acc(v[21], W[0] * e0 + W[3] * e1 + W[6] * e2);
  acc(v[22], W[1] * e0 + W[4] * e1 + W[7] * e2);
  acc(v[23], W[2] * e0 + W[5] * e1 + W[8] * e2);
  acc(v[24], Q[0] * e0 + Q[3] * e1 + Q[6] * e2);
  acc(v[25], Q[1] * e0 + Q[4] * e1 + Q[7] * e2);
  acc(v[26], Q[2] * e0 + Q[5] * e1 + Q[8] * e2);
  if constexpr (!ROBUST) acc(v[kCountSlot], 1.0);
}

constexpr uint32_t kMemoMiss = 0xFFFFFFFFu;  // memo.w of a point whose voxel is not in the map
constexpr uint32_t kMemoNone = 0xFFFFFFFEu;  // nothing looked up

// One VGICP round.  Launch j reads state j&1 and the rows launch j-1 wrote, writes state (j+1)&1
// and its own rows; the host alternates the buffers; the kernel boundary is the only synchronisation
// between workgroups.  Inside a workgroup wave 0 is the SOLVER (it owns no points); waves 1.. are
// workers, BLOCK-64 points per workgroup pass:
//   all      issue the loads of the previous rows, the state and (workers) the first point AND ITS MEMO; fold rows
//   solver   LDLT solve, exponential, compose, convergence -> new pose in LDS       } concurrently,
//   workers  fetch the payload of the voxel the memo names (nothing to compute)     } between two barriers
//   workers  transform with the NEW pose; "still inside last round's voxel?" (same_voxel_coord, the persistent launch's
//            test) — almost always yes: the payload is in registers, or the point is known to have no voxel and costs
//            nothing; a changed key is probed and remembered
//   workers  accumulate, grid-stride over further points, butterfly, one 256-byte row per workgroup.
// Round 6 brought the loop to the persistent launch's data path (it is what an RCCL communicator, a multi-device
// context after a give-up and every VGICP_FLAG_NO_PERSISTENT align run): a 16-byte MEMO per point in HBM {key, slot or
// index in the dense record copy} — the map is immutable during an align (src/LocalMap.cpp:94-100), so an unchanged
// key that missed costs 16 bytes instead of a 128-byte line, and one that hit goes straight to its payload (rounds
// 1-5 transformed with the OLD pose, hashed and probed every point in every launch: 1.66 x the algorithmic bytes at C2);
// nine instead of twelve planes of a scan whose covariances are all bitwise symmetric; the dense record copy of tables
// beyond the caches' reach.  The arithmetic per match is unchanged, so the loop still returns the persistent launch's bits.
// ROBUST: the weighted round of include/vgicp_hip_robust.h — an instantiation of its own, so that the plain one keeps its
// code; nothing but accumulate_match's contribution differs.
// PRIOR: the pose prior of include/vgicp_hip_prior.h — instantiations of their own again; nothing but the solve differs.
template <int BLOCK, bool ROBUST = false, bool PRIOR = false>
__global__ __launch_bounds__(BLOCK) void iterate_kernel(IterArgs a) {
  constexpr int kWaves = BLOCK / 64;
  constexpr int kWorkers = BLOCK - 64;
  __shared__ PrologueShared<BLOCK> sh;
  __shared__ double red[kWaves][kSlots];

  const uint64_t t_begin = a.stamps ? wall_clock64() : 0;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool worker = wave != 0;
  const uint32_t stride_pts = gridDim.x * kWorkers;
  const double inv_voxel = 1.0 / a.voxel_size;
  const double same_margin = 0x1p-20 * a.voxel_size;  // same_voxel_coord
  const bool cov_sym = scan_cov_symmetric(a);  // uniform
  const bool remembered = a.memo != nullptr && a.memo_valid != 0;           // uniform: an earlier launch of this align wrote the memos
  const VoxelRecord* pay_base = a.dense ? a.dense : a.table;                // uniform: where a remembered record's payload is read from
  RobustSetting robust;
  if constexpr (ROBUST) robust = robust_setting(a.robust.kernel, a.robust.scale2, a.robust.gate);  // uniform
  uint32_t i = worker ? blockIdx.x * kWorkers + (tid - 64) : a.n;

  double q[kScanPlanes];
#pragma unroll
  for (int k = 0; k < kScanPlanes; ++k) q[k] = 0.0;
  int4 m = make_int4(0, 0, 0, (int32_t)kMemoNone);
  if (i < a.n) {
    load_point_sym(a.scan, a.stride, i, q, cov_sym);
    if (remembered) m = a.memo[i];
  }

  int it, max_it;
  double cos_thr, tsq_thr;
  RoundHead head = prologue_fold<BLOCK>(a, sh, it, max_it, cos_thr, tsq_thr);
  if (head.stop) return;  // uniform across the grid: the loop ended in an earlier launch
  const bool solving = a.prev_rows != 0;  // uniform
  if (solving) __syncthreads();
  const uint64_t t_fold = a.stamps ? wall_clock64() : 0;

  // the payload the memo names (workers) || solve (wave 0)
  double mu[3] = {0.0, 0.0, 0.0}, S[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) S[k] = 0.0;
  bool have_payload = false;
  if (worker) {
    if (i < a.n && remembered && (uint32_t)m.w < kMemoNone) {
      load_payload(pay_base + (uint32_t)m.w, mu, S);
      have_payload = true;
    }
  } else if (solving) {
    prologue_solve<BLOCK, PRIOR>(a, sh, head.total, lane, it, max_it, cos_thr, tsq_thr);
    if (a.stamps && blockIdx.x == 0 && tid == 0)
      atomicAdd((unsigned long long*)&a.stamps[6], (unsigned long long)(wall_clock64() - t_fold));
  }
  if (solving) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) head.total.R[k] = sh.pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) head.total.t[k] = sh.pose[9 + k];
    head.stop = sh.stop != 0;
    if (head.stop) return;  // uniform: converged, or max_iteration reached
  }
  const uint64_t t_head = a.stamps ? wall_clock64() : 0;
  const double* R = head.total.R;
  const double* t = head.total.t;

  double v[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) v[k] = 0.0;

  bool first = true;
  while (i < a.n) {
    const double x = q[0], y = q[1], z = q[2];
    double C[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = q[3 + k];
    const uint32_t icur = i, inext = i + stride_pts;
    const int4 mcur = m;
    if (inext < a.n) {  // prefetch the next point (and its memo) under this one's gather
      load_point_sym(a.scan, a.stride, inext, q, cov_sym);
      if (remembered) m = a.memo[inext];
    }
    i = inext;

    double p[3];
    transform_point(R, t, x, y, z, p);
    bool hit;
    // still inside last round's voxel?  (true implies an unchanged key; the key itself is made only otherwise)
    const bool stayed = remembered && (uint32_t)mcur.w != kMemoNone &&
                        (((int)same_voxel_coord(p[0], mcur.x, a.voxel_size, same_margin) &
                          (int)same_voxel_coord(p[1], mcur.y, a.voxel_size, same_margin) &
                          (int)same_voxel_coord(p[2], mcur.z, a.voxel_size, same_margin)) != 0);
    if (stayed) {
      hit = (uint32_t)mcur.w != kMemoMiss;
      if (hit && !(first && have_payload)) load_payload(pay_base + (uint32_t)mcur.w, mu, S);
    } else {
      const int32_t kx = voxel_coord_fast(p[0], a.voxel_size, inv_voxel);
      const int32_t ky = voxel_coord_fast(p[1], a.voxel_size, inv_voxel);
      const int32_t kz = voxel_coord_fast(p[2], a.voxel_size, inv_voxel);
      if (remembered && (uint32_t)mcur.w != kMemoNone && mcur.x == kx && mcur.y == ky && mcur.z == kz) {
        hit = (uint32_t)mcur.w != kMemoMiss;   // a point right below a face: key unchanged after all
        if (hit && !(first && have_payload)) load_payload(pay_base + (uint32_t)mcur.w, mu, S);
      } else {
        const VoxelRecord* rec = find_voxel(a.table, a.mask, kx, ky, kz);
        hit = rec != nullptr;
        if (a.memo) {
          uint32_t where = kMemoMiss;
          if (hit) where = a.dense ? reinterpret_cast<const uint32_t*>(&rec->reserved)[1] : (uint32_t)(rec - a.table);
          a.memo[icur] = make_int4(kx, ky, kz, (int32_t)where);
        }
        if (hit) load_payload(rec, mu, S);
      }
    }
    if (hit) {
      if (first) accumulate_match<true, ROBUST>(R, p, C, mu, S, v, robust);  // the thread's first point of the round
      else accumulate_match<false, ROBUST>(R, p, C, mu, S, v, robust);
    }
    first = false;
  }
  const uint64_t t_loop = a.stamps ? wall_clock64() : 0;

  if (worker) wave_fold_to_lds(v, lane, red[wave]);
  __syncthreads();
  // one plain 256-byte row per workgroup
  if (tid < kSlots) {
    double w_sum[kWaves - 1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) w_sum[w - 1] = red[w][tid];
    a.rows[(size_t)blockIdx.x * kSlots + tid] = tree_sum<kWaves - 1>(w_sum);
  }
  if (a.stamps && blockIdx.x == 0 && tid == 64) {
    const uint64_t t_end = wall_clock64();
    atomicAdd((unsigned long long*)&a.stamps[0], (unsigned long long)(t_fold - t_begin));
    atomicAdd((unsigned long long*)&a.stamps[5], (unsigned long long)(t_head - t_fold));
    atomicAdd((unsigned long long*)&a.stamps[1], (unsigned long long)(t_loop - t_head));
    atomicAdd((unsigned long long*)&a.stamps[2], (unsigned long long)(t_end - t_loop));
    atomicAdd((unsigned long long*)&a.stamps[4], 1ull);
  }
}

// The launch after the last round: prologue only (fold the last rows, solve, publish the final
// state), one workgroup.  A kernel of its own so per-kernel profiles of iterate_kernel hold rounds only.
template <int BLOCK, bool PRIOR = false>
__global__ __launch_bounds__(BLOCK) void close_kernel(IterArgs a) {
  __shared__ PrologueShared<BLOCK> sh;
  int it, max_it;
  double cos_thr, tsq_thr;
  const RoundHead head = prologue_fold<BLOCK>(a, sh, it, max_it, cos_thr, tsq_thr);
  if (head.stop || a.prev_rows == 0) return;
  __syncthreads();
  if (threadIdx.x < 64) prologue_solve<BLOCK, PRIOR>(a, sh, head.total, threadIdx.x, it, max_it, cos_thr, tsq_thr);
}

// Scoring poses of the resident scan (vgicp_evaluate_resident, include/vgicp_hip_evaluate.h): what round 0 of the loop
// accumulates at a pose, for several poses in one launch, plus the objective and the squared error in two spare slots.
// Grid: (rows per pose) x (poses), the pose index the SLOW dimension, so that workgroups of different poses that run
// side by side read the same scan lines and table records.  Workgroup (vb, h) is workgroup vb of iterate_kernel<BLOCK>'s
// first launch from pose h on a grid of gridDim.x: waves 1.. own points, grid-stride, the same `first` rule, the same
// butterfly, LDS step and tree_sum — so its row's slots 0-27 are that launch's row vb, bit for bit.  No memo, no dense
// copy, no state: nothing is written but the rows, nothing waits for another workgroup.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void evaluate_kernel(EvalArgs a) {
  constexpr int kWaves = BLOCK / 64;
  constexpr int kWorkers = BLOCK - 64;
  __shared__ double red[kWaves][kSlots];

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool worker = wave != 0;
  const uint32_t stride_pts = gridDim.x * kWorkers;
  const double inv_voxel = 1.0 / a.voxel_size;
  const bool cov_sym = scan_cov_symmetric(a);  // uniform
  uint32_t i = worker ? blockIdx.x * kWorkers + (tid - 64) : a.n;

  double q[kScanPlanes];
#pragma unroll
  for (int k = 0; k < kScanPlanes; ++k) q[k] = 0.0;
  if (i < a.n) load_point_sym(a.scan, a.stride, i, q, cov_sym);

  const double* pose = a.poses + (size_t)blockIdx.y * 12;  // uniform: R column-major (9) then t (3)
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = pose[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = pose[9 + k];

  double v[kSlots];
#pragma unroll
  for (int k = 0; k < kSlots; ++k) v[k] = 0.0;

  bool first = true;
  while (i < a.n) {
    const double x = q[0], y = q[1], z = q[2];
    double C[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = q[3 + k];
    const uint32_t inext = i + stride_pts;
    if (inext < a.n) load_point_sym(a.scan, a.stride, inext, q, cov_sym);  // the next point under this one's gather
    i = inext;

    double p[3];
    transform_point(R, t, x, y, z, p);
    const int32_t kx = voxel_coord_fast(p[0], a.voxel_size, inv_voxel);
    const int32_t ky = voxel_coord_fast(p[1], a.voxel_size, inv_voxel);
    const int32_t kz = voxel_coord_fast(p[2], a.voxel_size, inv_voxel);
    const VoxelRecord* rec = find_voxel(a.table, a.mask, kx, ky, kz);
    if (rec != nullptr) {
      double mu[3], S[9];
      load_payload(rec, mu, S);
      if (first) accumulate_match<true>(R, p, C, mu, S, v);
      else accumulate_match<false>(R, p, C, mu, S, v);
      // S now holds R C R^T + C_voxel: W again from it (the inverse match_weight ended with; the compiler merges the
      // two), and the cost by mahalanobis, the definition the robust round and point_term use
      double W[9];
      inverse3_cofactor(S, W);
      const double e0 = p[0] - mu[0], e1 = p[1] - mu[1], e2 = p[2] - mu[2];
      v[kCostSlot] += mahalanobis(W, e0, e1, e2);
      v[kSqErrorSlot] += e0 * e0 + e1 * e1 + e2 * e2;
    }
    first = false;
  }

  if (worker) wave_fold_to_lds(v, lane, red[wave]);
  __syncthreads();
  if (tid < kSlots) {
    double w_sum[kWaves - 1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) w_sum[w - 1] = red[w][tid];
    a.rows[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kSlots + tid] = tree_sum<kWaves - 1>(w_sum);
  }
}

// The fold of iterate_kernel<512>'s prologue (prologue_fold + the first lines of prologue_solve) over the rows of one
// pose per workgroup: 16 groups of threads add the rows group, group + 16, ... as tree_sum<16> batches (rows beyond the
// pose's count +0.0 in their place), then tree_sum<16> over the groups.  All 32 slots; one 256-byte row per pose, written
// straight into the page-locked result.
__global__ __launch_bounds__(512) void evaluate_fold_kernel(const double* __restrict__ rows, uint32_t rows_per_pose,
                                                            double* __restrict__ out) {
  constexpr int kGroups = 512 / kSlots;
  constexpr int kBatch = 16;
  __shared__ double fin[kGroups][kSlots];
  const uint32_t tid = threadIdx.x, slot = tid & (kSlots - 1), group = tid / kSlots;
  const double* prev = rows + (size_t)blockIdx.x * rows_per_pose * kSlots;
  double row[kBatch];
#pragma unroll
  for (int u = 0; u < kBatch; ++u) {
    const uint32_t b = group + u * kGroups;
    row[u] = b < rows_per_pose ? prev[(size_t)b * kSlots + slot] : 0.0;
  }
  double s = tree_sum<kBatch>(row);
  for (uint32_t b0 = group + kBatch * kGroups; b0 < rows_per_pose; b0 += kGroups * kBatch) {
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const uint32_t b = b0 + u * kGroups;
      row[u] = b < rows_per_pose ? prev[(size_t)b * kSlots + slot] : 0.0;
    }
    s += tree_sum<kBatch>(row);
  }
  fin[group][slot] = s;
  __syncthreads();
  if (tid < kSlots) {
    double part[kGroups];
#pragma unroll
    for (int g = 0; g < kGroups; ++g) part[g] = fin[g][tid];
    out[(size_t)blockIdx.x * kSlots + tid] = tree_sum<kGroups>(part);
  }
}

// The term of point i, for point_terms_kernel and gate_decide_kernel (the view both argument structs begin with): the
// point, ONE find_voxel probe, the payload, then match_weight and mahalanobis — the definition the rounds and the
// evaluation call, so d^2 here is the evaluation's cost term and the robust round's raw residual.
struct PointTerm {
  double raw, sq;   // e^T W e and |e|^2; +infinity when the point's voxel is not in the map
  bool matched;
};
__device__ __forceinline__ PointTerm point_term(const PoseView& a, uint32_t i, bool cov_sym) {
  double q[kScanPlanes];
  load_point_sym(a.scan, a.stride, i, q, cov_sym);
  double R[9], t[3], C[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { R[k] = a.pose[k]; C[k] = q[3 + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = a.pose[9 + k];
  const double inv_voxel = 1.0 / a.voxel_size;
  double p[3];
  transform_point(R, t, q[0], q[1], q[2], p);
  const int32_t kx = voxel_coord_fast(p[0], a.voxel_size, inv_voxel);
  const int32_t ky = voxel_coord_fast(p[1], a.voxel_size, inv_voxel);
  const int32_t kz = voxel_coord_fast(p[2], a.voxel_size, inv_voxel);
  const VoxelRecord* rec = find_voxel(a.table, a.mask, kx, ky, kz);
  PointTerm term{__builtin_inf(), __builtin_inf(), false};
  if (rec != nullptr) {
    term.matched = true;
    double mu[3], S[9];
    load_payload(rec, mu, S);
    double W[9];
    match_weight(R, C, S, W);
    const double e0 = p[0] - mu[0], e1 = p[1] - mu[1], e2 = p[2] - mu[2];
    term.raw = mahalanobis(W, e0, e1, e2);
    term.sq = e0 * e0 + e1 * e1 + e2 * e2;
  }
  return term;
}

// The resident scan at a pose, point by point (vgicp_points_resident, include/vgicp_hip_points.h).  One point per
// thread, 256 threads: the point's term by point_term (match_weight and mahalanobis, as accumulate_match<..., ROBUST>
// and evaluate_kernel call them) — without the 27 sums, so nothing is reduced but four counts.  The requested planes are
// written at the point's index:
// every store of a wave is one coalesced access.  A point's values depend on nothing but the point, the pose and the
// settings: not on which planes are asked, not on its neighbours.  Nothing waits for another workgroup.
__global__ __launch_bounds__(256) void point_terms_kernel(PointArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool cov_sym = scan_cov_symmetric(a);  // uniform
  const RobustSetting robust = robust_setting(a.robust_kernel, a.robust_scale2, a.robust_gate);
  bool matched = false, counted = false, negative = false, not_finite = false;
  if (i < a.n) {
    const PointTerm term = point_term(a, i, cov_sym);
    const double raw = term.raw, sq = term.sq;
    double w = 0.0;
    if (term.matched) {
      matched = true;
      w = robust_weight(robust, raw);
      counted = w > 0.0;
      not_finite = !(fabs(raw) < __builtin_inf());
      negative = !not_finite && raw < 0.0;
    }
    if (a.d2) a.d2[i] = raw;
    if (a.sq_error) a.sq_error[i] = sq;
    if (a.weight) a.weight[i] = w;
    if (a.status) a.status[i] = (uint8_t)((matched ? 1u : 0u) | (negative ? 2u : 0u) | (not_finite ? 4u : 0u));
    if (a.keys) {
      a.keys[i] = matched && !not_finite ? point_key(raw) : kPointKeyUnranked;
      a.idx[i] = i;
    }
  }
  // one atomic per workgroup and counter, as insert_prepare_kernel counts
  const int c_matched = __syncthreads_count(matched ? 1 : 0);
  const int c_counted = __syncthreads_count(counted ? 1 : 0);
  const int c_negative = __syncthreads_count(negative ? 1 : 0);
  const int c_not_finite = __syncthreads_count(not_finite ? 1 : 0);
  if (threadIdx.x == 0) {
    if (c_matched) atomicAdd(&a.counters[0], (uint32_t)c_matched);
    if (c_counted) atomicAdd(&a.counters[1], (uint32_t)c_counted);
    if (c_negative) atomicAdd(&a.counters[2], (uint32_t)c_negative);
    if (c_not_finite) atomicAdd(&a.counters[3], (uint32_t)c_not_finite);
  }
}

// The decision of a gated map insertion (GateArgs, vgicp_device.h): the same point, probe and term, and one keep byte.
// A point is refused iff it is matched and not max(raw, 0) <= gate: a NaN or infinite raw fails the comparison at every
// gate, a negative raw counts as 0, an unmatched point opens new ground and is kept.  Read-only on the table and
// waiting on nothing: the claims of the insertion are a later launch, so no claim in flight is ever seen here.
__global__ __launch_bounds__(256) void gate_decide_kernel(GateArgs a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool cov_sym = scan_cov_symmetric(a);  // uniform
  bool matched = false, refused = false, not_finite = false;
  if (i < a.n) {
    const PointTerm term = point_term(a, i, cov_sym);
    matched = term.matched;
    if (matched) {
      not_finite = !(fabs(term.raw) < __builtin_inf());
      refused = not_finite || !(fmax(term.raw, 0.0) <= a.gate);
    }
    a.keep[i] = refused ? (uint8_t)0 : (uint8_t)1;
  }
  const int c_matched = __syncthreads_count(matched ? 1 : 0);
  const int c_refused = __syncthreads_count(refused ? 1 : 0);
  const int c_not_finite = __syncthreads_count(not_finite ? 1 : 0);
  if (threadIdx.x == 0) {
    if (c_matched) atomicAdd(&a.counters[0], (uint32_t)c_matched);
    if (c_refused) atomicAdd(&a.counters[1], (uint32_t)c_refused);
    if (c_not_finite) atomicAdd(&a.counters[2], (uint32_t)c_not_finite);
  }
}

// The pick: one wave.  m = matched - not finite is read here, on the device; lane j takes quantile j: its rank by
// quantile_rank (vgicp_points_plan.h, the definition) and the sorted key there, whose pattern IS the value.  The ranked
// points sort in front of the others, so a rank below m names one of them.  Counts and quantiles go straight into
// page-locked memory.
__global__ __launch_bounds__(64) void point_pick_kernel(PointPickArgs a) {
  const uint32_t lane = threadIdx.x;
  if (lane < (uint32_t)kPointCounters) a.out[lane] = a.counters[lane];
  if (lane < a.n_quantiles && lane < (uint32_t)kPointQuantiles) {
    const uint32_t matched = a.counters[0], not_finite = a.counters[3];
    const uint64_t m = matched > not_finite ? matched - not_finite : 0u;
    unsigned long long bits = 0x7FF8000000000000ull;   // NaN: nothing is ranked
    if (m > 0) {
      const uint64_t rank = quantile_rank(a.q[lane], m);
      if (rank < a.n) bits = a.sorted[rank];
    }
    a.out[kPointCounters + lane] = bits;
  }
}

// Test hook (vgicp_solve_step): the tail of one round on given normal equations, run by ONE wave with
// the very device functions the loop kernels inline — JTJ.ldlt().solve(-JTr), Utils::se3ToSE3 and
// ICP::convergenceCheck (src/Registration.cpp:78-79,37-50, src/Utils.cpp:40-63).
// packed: 21 lower-triangle entries row by row, then the 6 entries of JTr.
// out: [0..5] se3, [6..14] step R (column-major), [15..17] step t, [18] 1.0 when the pivoted
// (Eigen-faithful) solve produced the result, [19] 1.0 when the step passes the convergence test.
__global__ __launch_bounds__(64) void solve_step_kernel(const double* __restrict__ packed, double cos_thr,
                                                        double tsq_thr, int force_pivoted,
                                                        double* __restrict__ out) {
  __shared__ double totals[kSlots];
  __shared__ double work[kSolveWork];
  const uint32_t lane = threadIdx.x;
  if (lane < kSlots) totals[lane] = lane < kNormalEq ? packed[lane] : 0.0;
  __syncthreads();
  double A[21], g[6], xi[6];
#pragma unroll
  for (int k = 0; k < 21; ++k) A[k] = packed[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) g[k] = -packed[21 + k];
  bool pivoted = force_pivoted != 0;
  if (pivoted || !ldlt6_solve_spd(A, g, xi)) {  // uniform branch
    ldlt6_solve_pivoted(totals, work, lane, xi);
    pivoted = true;
  }
  Pose step;
  se3_exp_device(xi, step);
  const bool conv = converged(step, cos_thr, tsq_thr);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = xi[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) out[6 + k] = step.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[15 + k] = step.t[k];
    out[18] = pivoted ? 1.0 : 0.0;
    out[19] = conv ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------
// Persistent variant: the whole loop of ICP::align (src/Registration.cpp:15-28) in ONE launch.
//
// Same arithmetic, same fixed summation orders and the same workgroup geometry as iterate_kernel<512>
// (so both variants return the same bits); what changes is how a round's partial rows travel.  There is
// no flag, no counter and no drain on the path: the DATA is the signal.  Every 8-byte word of the exchange
// buffers holds kRowUnset until its producer stores the value with ONE write-through (sc1) 8-byte store —
// a naturally aligned granule written by one store is never seen torn (MI355X_MICROARCH.md, "R2's granule")
// — and consumers poll the words they need with sc1 loads until none is kRowUnset:
//   level 1  wave 0 of workgroup b stores its row (28 words).  Folder g (= workgroup g < 16) polls the rows
//            b = g, g + 16, g + 32 ... (lane = slot, up to 16 loads in flight), adds them in ascending b and
//            stores the part
//   level 2  wave 0 of EVERY workgroup polls the <= 16 parts, adds them in ascending g, solves
// which is the order in which prologue_fold / prologue_solve add the rows (thread (g, slot) adds rows
// g + 16u, then the 16 group sums are added in ascending g).  Two one-way hops instead of store + drain +
// atomic + poll + row read, 57 KB less to read per workgroup and round, and two workgroup barriers per
// round instead of five.
// Re-arming (three buffers by round % 3): at the end of round j (all parts of round j seen) a workgroup
// stores kRowUnset over its row and, if a folder, its part of buffer (j - 1) % 3.  Safe: every part of
// round j exists, so every row of round j was published, so every workgroup had finished reading round
// j - 1.  Ordered: the producer's next publication (round j + 1) waits for its own stores to complete
// first (s_waitcnt vmcnt(0)), and a consumer polls buffer (j - 1) % 3 again only in round j + 2, after it
// has seen a part of round j + 1 that depends on that publication.  Nothing is tidied up when a launch ends: the
// round number runs on from launch to launch (PersistArgs::round0 = rounds executed on this context before), so the
// next launch's first rounds re-arm what this launch published last — every workgroup of that launch has published
// by then, hence left this launch and its reads behind.  There is no exit counter and no last arriver.
// What stays on chip across rounds: a thread's first point with the voxel record it used (registers);
// for scans larger than the grid, per further point its last key and table slot (16-byte memo in LDS: an
// unchanged key that missed costs no table access at all — the map is immutable during align,
// src/LocalMap.cpp:94-100 — and one that hit loads its payload straight from the slot), and up to
// stash_points whole points (LDS).
// Needs every workgroup resident (grid <= CUs, one 512-thread workgroup per CU); a poll that exceeds
// spin_limit ends the kernel without the final state, and the host re-runs the align with iterate_kernel.
typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;

__device__ __forceinline__ void store_through_bits(double* p, unsigned long long bits) {
  __hip_atomic_store((gu64*)p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long load_through_bits(const double* p) {
  return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Mailbox words live in fine-grained memory of this or another GPU: system scope (sc0 sc1) both ways.
__device__ __forceinline__ void store_system_bits(double* p, unsigned long long bits) {
  __hip_atomic_store((gu64*)p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned long long load_system_bits(const double* p) {
  return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// A sum as it is published: never the "unset" pattern (a NaN with that payload can only come from
// non-finite input; it is published as the canonical NaN and the align ends as VGICP_ERR_DEGENERATE).
__device__ __forceinline__ unsigned long long publishable(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return b == kRowUnset ? kRowNaN : b;
}

constexpr int kL2Delay = 64;   // s_sleep units (64 clocks each) a workgroup that is no folder waits before its first poll of the parts
// Lanes <= kCountSlot (lane = slot) end with the sum over the 16 consecutive rows at src, as the pairwise tree over
// ascending rows (tree_sum<16>, as the folds of iterate_kernel do; rows that belong to no workgroup hold +0.0 for
// good).  All 64 lanes of the wave call it; false when spin_limit polls did not suffice.
// The two halves of the wave share the work (round 6): lane l < 32 polls rows 0..7 of slot l, lane l + 32 rows 8..15, and
// tree_sum<16> IS tree_sum<8>(first half) + tree_sum<8>(second half), so one half-swap gives the same bits with half the
// registers and half the loads per lane.  ONE poll of the eight words is in flight: two, three or four of them, issued a
// fraction of a memory round trip apart so that a word which lands just after a poll has passed need not wait a whole
// round trip for the next, made every round SLOWER (C2 +0.3 / +0.9 / +1.5 us: the polls of 256 workgroups queue at the
// memory side, profiles/NOTES_dropped_experiments.md) — which is what led to kL2Delay: poll LESS.
// LIVE (the team launch): only the first `live` of the 16 rows belong to a workgroup; the others are taken as +0.0
// without a load — the value the single launch finds there — and are added in their place of the tree all the same.
template <bool SYSTEM, bool LIVE = false>
__device__ __forceinline__ bool poll_and_sum(const double* src, uint32_t lane, uint32_t spin_limit, double& sum,
                                             uint32_t live = (uint32_t)kFolders) {
  constexpr int H = kFolders / 2;
  const uint32_t slot = lane & 31u, half = lane >> 5;
  const bool active = slot <= (uint32_t)kCountSlot;
  const double* mine = src + (size_t)half * H * kSlots + (active ? slot : 0u);
  unsigned long long w[H];
  if constexpr (LIVE) {
#pragma unroll
    for (int k = 0; k < H; ++k)   // a word that is not live is never kRowUnset, so the loop below leaves it alone
      w[k] = (active && half * H + (uint32_t)k < live) ? load_through_bits(mine + k * kSlots) : 0ull;
  } else {
#pragma unroll
    for (int k = 0; k < H; ++k)
      w[k] = active ? (SYSTEM ? load_system_bits(mine + k * kSlots) : load_through_bits(mine + k * kSlots)) : 0ull;
  }
  for (uint32_t spins = 0;; ++spins) {
    bool missing = false;
#pragma unroll
    for (int k = 0; k < H; ++k) missing = missing || (w[k] == kRowUnset);
    if (!__any(missing)) break;
    if (spins >= spin_limit) return false;
    __builtin_amdgcn_s_sleep(1);
#pragma unroll
    for (int k = 0; k < H; ++k)
      if (w[k] == kRowUnset) w[k] = SYSTEM ? load_system_bits(mine + k * kSlots) : load_through_bits(mine + k * kSlots);
  }
  double x[H];
#pragma unroll
  for (int k = 0; k < H; ++k) x[k] = __longlong_as_double((long long)w[k]);
  const double part = tree_sum<H>(x);
  // lanes < 32 receive the sum of lane + 32 (rows 8..15 of the same slot)
  const unsigned plo = (unsigned)__double2loint(part), phi = (unsigned)__double2hiint(part);
  const auto lo = __builtin_amdgcn_permlane32_swap(plo, plo, false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(phi, phi, false, false);
  sum = part + __hiloint2double((int)hi[1], (int)lo[1]);
  return true;
}

// STAMPS builds only: a clock reading that cannot move across the values it is given (they pass through an empty asm)
template <int N>
__device__ __forceinline__ uint64_t pinned_clock(double (&x)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+v"(x[k]));
  const uint64_t t = wall_clock64();
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+v"(x[k]));
  return t;
}

// A staged unit's flag line as the host's copy thread leaves it: flags[16 u] = the sequence number, flags[16 u + 1] = the
// form of its covariances, stored BEFORE the flag.  Both lie in one naturally aligned 8-byte granule, so one system-scope
// load brings both over the link: the low word is the flag, and when it says `seq` the high word is that unit's form (a
// second, dependent load of the form would cost another PCIe read latency per unit).
__device__ __forceinline__ unsigned long long load_flag_and_form(const uint32_t* flags, uint32_t u) {
  return __hip_atomic_load((gu64*)(flags + 16 * (size_t)u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Where a workgroup of the fused align leaves the resident copy of its points (fused_leave_resident): written to LDS by
// fused_round0_load and read back inside round 0, so that none of it occupies registers across the round loop.
struct FusedLeave {
  double* plane;     // SoA: plane 0 at the workgroup's first point
  double* aos_pts;   // AoS copy, at the workgroup's first point
  double* aos_cov;
  uint32_t* asym;
  uint64_t stride;
  uint32_t seq, cnt; // cnt: the workgroup's points
};

// The fused align's round-0 load (all threads of the workgroup; one point per worker thread).  The workgroup's 448
// points lie in one or two staged units: thread 0 waits for their flags with system-scope loads and the pack's patience,
// then the workgroup reads the points and the covariances over PCIe as pack_arena_kernel does — contiguous 16-byte
// non-temporal loads into LDS (`lds`: 18 x 448 doubles, the neighbour-prefetch area, unused before round 0), the
// compact or full form per unit, the odd-count tail read whole (the staging areas are padded).  Each worker thread
// returns its point in q0, as load_point would have read it from the planes; what the pack left behind for these
// points is stored later, out of lds[0 .. 12 x 448), to the addresses noted in *leave (fused_leave_resident).  false: a
// unit did not arrive in time.
__device__ __forceinline__ bool fused_round0_load(const FusedUpload& f, uint64_t stride, uint32_t n_pts, double* lds,
                                                  FusedLeave* leave, double (&q0)[kScanPlanes]) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  constexpr uint32_t B = 512, W = B - 64;   // the persistent workgroup and its worker threads
  __shared__ uint32_t ok_sh, form_sh[2];
  const uint32_t tid = threadIdx.x, p0 = blockIdx.x * W;
  const uint32_t cnt = p0 < n_pts ? min(W, n_pts - p0) : 0u;  // uniform
  if (tid == 0) {   // read behind round 0's first barrier
    leave->plane = f.soa + p0;
    leave->aos_pts = f.aos_pts + 3 * (size_t)p0;
    leave->aos_cov = f.aos_cov + 9 * (size_t)p0;
    leave->asym = f.asym;
    leave->stride = stride;
    leave->seq = f.seq;
    leave->cnt = cnt;
  }
  if (cnt == 0) return true;
  const uint32_t ua = p0 / f.unit, ub = (p0 + cnt - 1) / f.unit;  // W < unit: at most two units
  const uint32_t split = min(p0 + cnt, (ua + 1) * f.unit);         // the first point of unit ub (p0 + cnt: one unit)
  if (tid == 0) {
    uint32_t good = 1;
    for (uint32_t u = ua; u <= ub && good; ++u) {
      unsigned long long w = load_flag_and_form(f.flags, u);
      for (uint32_t spins = 0; (uint32_t)w != f.seq; ++spins) {
        if (spins >= f.spin_limit) { good = 0; break; }
        __builtin_amdgcn_s_sleep(20);
        w = load_flag_and_form(f.flags, u);
      }
      form_sh[u == ua ? 0 : 1] = (uint32_t)(w >> 32);   // the form that came with the flag
    }
    if (ua == ub) form_sh[1] = form_sh[0];
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    ok_sh = good;
  }
  __syncthreads();
  if (!ok_sh) return false;  // uniform
  double* lp = lds;             // points: 3 x W
  double* lc = lds + 3 * W;     // covariances, whole records: 9 x W
  double* lq = lds + 12 * W;    // compact records as staged: 6 x W
  {
    const v4i* sp = reinterpret_cast<const v4i*>(f.apts + (size_t)p0 * 24);
    const uint32_t np = (cnt * 24 + 15) / 16;
    for (uint32_t k = tid; k < np; k += B) reinterpret_cast<v4i*>(lp)[k] = __builtin_nontemporal_load(sp + k);
  }
  for (uint32_t s = 0; s < 2; ++s) {
    // a segment starts at p0 or at a unit's start, both even: 16-byte aligned in the staging memory and in LDS
    const uint32_t s0 = s ? split : p0, s1 = s ? p0 + cnt : split, u = s ? ub : ua;  // uniform
    if (s0 >= s1) continue;
    if (form_sh[s] == kArenaCompact) {
      const v4i* sc = reinterpret_cast<const v4i*>(f.acov + (size_t)u * f.unit * 72 + (size_t)(s0 - u * f.unit) * 48);
      v4i* dst = reinterpret_cast<v4i*>(lq + 6 * (s0 - p0));
      for (uint32_t k = tid; k < (s1 - s0) * 3; k += B) dst[k] = __builtin_nontemporal_load(sc + k);
    } else {
      const v4i* sc = reinterpret_cast<const v4i*>(f.acov + (size_t)s0 * 72);
      v4i* dst = reinterpret_cast<v4i*>(lc + 9 * (s0 - p0));
      const uint32_t nc = ((s1 - s0) * 72 + 15) / 16;
      for (uint32_t k = tid; k < nc; k += B) dst[k] = __builtin_nontemporal_load(sc + k);
    }
  }
  __syncthreads();
  if (tid < cnt && form_sh[p0 + tid >= split ? 1 : 0] == kArenaCompact) {  // the three mirrored entries are made here
    const double* q = lq + 6 * tid;
    const double a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], a5 = q[5];
    double* c = lc + 9 * tid;
    c[0] = a0; c[1] = a1; c[2] = a2; c[3] = a1; c[4] = a3; c[5] = a4; c[6] = a2; c[7] = a4; c[8] = a5;
  }
  __syncthreads();
  // the workgroup's points have crossed the link: where the registration's device time starts (the two-launch path's
  // persistent launch starts with every point packed)
  if (tid == 0) atomicMax(f.unit_clock, (unsigned long long)wall_clock64());
  const uint32_t wt = tid - 64u;
  if (tid >= 64u && wt < cnt) {
#pragma unroll
    for (int k = 0; k < 3; ++k) q0[k] = lp[3 * wt + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) q0[3 + k] = lc[9 * wt + k];
  }
  return true;
}

// The resident copy of the workgroup's points, left behind by its WORKER threads (tid >= 64) once round 0's row is on its
// way: the 12 SoA planes and the AoS device copy, both coalesced out of the LDS that fused_round0_load filled
// (lds[0 .. 12 x 448) is untouched until the neighbour look-ahead first writes there, a round later), and the asymmetry
// word (from q0).  This launch never reads any of it again, so every word is stored write-through: nothing of the
// 86 KB per workgroup stays dirty in L2 for the end of the launch to write back, and nothing of it stands between the
// unit's arrival and round 0's voxel probe.  Eight bytes per lane and store: the odd count needs no tail.
__device__ __forceinline__ void fused_leave_resident(const FusedLeave* leave, const double* lds, const double (&q0)[kScanPlanes]) {
  constexpr uint32_t W = 512 - 64;
  // the addresses are made HERE, from the note in LDS (the empty asm keeps the lane's part from being hoisted out of the
  // round loop): kept in registers through every round they push the solver's constants into scratch
  uint32_t tid_here = threadIdx.x;
  asm volatile("" : "+v"(tid_here));
  const uint32_t wt = tid_here - 64u;
  const FusedLeave to = *leave;
  const double* lp = lds;
  const double* lc = lds + 3 * W;
  if (wt < to.cnt) {
    // plane by plane out of LDS, one address at a time
    double* plane = to.plane + wt;
#pragma unroll 1
    for (int k = 0; k < 3; ++k, plane += to.stride) store_through_bits(plane, (unsigned long long)__double_as_longlong(lp[3 * wt + k]));
#pragma unroll 1
    for (int k = 0; k < 9; ++k, plane += to.stride) store_through_bits(plane, (unsigned long long)__double_as_longlong(lc[9 * wt + k]));
    const bool same = __double_as_longlong(q0[4]) == __double_as_longlong(q0[6]) &&
                      __double_as_longlong(q0[5]) == __double_as_longlong(q0[9]) &&
                      __double_as_longlong(q0[8]) == __double_as_longlong(q0[10]);
    if (!same) *to.asym = to.seq;
  }
#pragma unroll 1
  for (uint32_t k = wt; k < 3 * to.cnt; k += W) store_through_bits(to.aos_pts + k, (unsigned long long)__double_as_longlong(lp[k]));
#pragma unroll 1
  for (uint32_t k = wt; k < 9 * to.cnt; k += W) store_through_bits(to.aos_cov + k, (unsigned long long)__double_as_longlong(lc[k]));
}

// MULTI: several GPUs (the rank totals cross xGMI through mailboxes); STAMPS: in-kernel phase clocks
// (VGICP_DEBUG_STAMPS=1).  Separate instantiations: the single-GPU production kernel carries neither.
// MANY: a thread owns several points (scan larger than grid x 448), wave 0 included; every point has a memo in LDS, the
// thread's first point stays in registers (its voxel record does not), some more are parked in LDS.  !MANY: one point
// per thread (waves 1..7), kept in registers together with the
// voxel record it used, plus the neighbour prefetch.  Separate instantiations keep both within 256 VGPRs.
// FUSED: round 0's points arrive through the staging memory of the upload (fused_round0_load), !MANY, !MULTI, !STAMPS.
// TEAM: one of several hypotheses that share a launch (TeamArgs in vgicp_device.h): the workgroup's index inside its team
// stands where blockIdx.x stands otherwise, the exchange words are the team's own, !MANY, !MULTI, !STAMPS, !FUSED.
struct TeamView {
  uint32_t vb = 0;           // index of the workgroup inside its team
  uint32_t team_wgs = 0;     // T
  uint32_t folder_rows = 0;  // U
  uint32_t* abort_word = nullptr;
};
// ROBUST: the weighted round (include/vgicp_hip_robust.h), single device, !STAMPS, !FUSED, !TEAM: accumulate_match's
// contribution takes the weight, everything else is the plain body's.
// PRIOR: the pose prior (include/vgicp_hip_prior.h), the robust round's scope: the solver section solves with
// prior_solve_totals' sums, everything else is the plain (or the robust) body's.
template <int BLOCK, bool MULTI, bool STAMPS, bool MANY, bool FUSED = false, bool TEAM = false, bool ROBUST = false,
          bool PRIOR = false>
__device__ __forceinline__ void persistent_body(const PersistArgs& a, const FusedUpload& up, const TeamView& tv = TeamView()) {
  static_assert(!ROBUST || (!MULTI && !STAMPS && !FUSED && !TEAM), "the robust round runs the single-device bodies only");
  static_assert(!PRIOR || (!MULTI && !STAMPS && !FUSED && !TEAM), "the pose prior runs the single-device bodies only");
  static_assert(!FUSED || (!MULTI && !STAMPS && !MANY), "the fused upload serves the single-device one-point-per-thread body");
  static_assert(!TEAM || (!MULTI && !STAMPS && !MANY && !FUSED), "teams run the single-device one-point-per-thread body");
  static_assert(BLOCK / kSlots == kFolders, "the exchange reproduces the fold order of iterate_kernel<512>");
  constexpr int kWaves = BLOCK / 64;
  constexpr int kWorkers = BLOCK - 64;
  __shared__ double red[kWaves][kSlots];
  __shared__ double totals[kSlots];
  __shared__ double work[kSolveWork];
  __shared__ double pose_sh[12];
  __shared__ int stop_sh;
  __shared__ FusedLeave leave_sh;   // FUSED only
  // Scans larger than the grid: a thread owns several points. The first stays in registers; of the
  // others, the first a.memo_points have a 16-byte memo {key, slot} and the first a.stash_points are
  // parked whole after round 0 (plane-major per point: conflict-free), so only the rest is re-read.
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
  // Scans that fit the grid (one point per thread, no memo / stash): the same LDS holds, per thread, the voxel
  // BEHIND THE NEAREST FACE of the point's voxel, looked up while the workers wait for the exchange: key + slot
  // (int4) and the 96-byte payload (6 planes of double2).  A point that changes voxel next round usually
  // enters exactly that one and finds its record (or the news that there is none) here.
  int4* pf_key = reinterpret_cast<int4*>(dyn_lds);
  double2* pf_pay = reinterpret_cast<double2*>(dyn_lds + (size_t)kWorkers * sizeof(int4));
  const bool prefetch = !MANY && a.prefetch_margin > 0.0;  // uniform

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // a.n bounds the count the device holds (a scan preparation that gave up must not send this launch out of range)
  const uint32_t n_pts = a.n_dev ? (*a.n_dev < a.n ? *a.n_dev : a.n) : a.n;  // uniform
  const bool cov_sym = MANY && scan_cov_symmetric(a);  // uniform
  const uint32_t grid = gridDim.x, blk = TEAM ? tv.vb : blockIdx.x;
  // MANY (the scan, or the upper bound the launch plan was made from, has more points than grid x 448): a thread owns
  // several points anyway, so wave 0 owns points as well and turns solver after the accumulate phase — 512 points
  // per workgroup pass instead of 448, two point-carrying waves on every SIMD instead of 2/2/2/1.
  constexpr uint32_t W = MANY ? (uint32_t)BLOCK : (uint32_t)kWorkers;  // point-carrying threads of a workgroup
  const bool worker = MANY || wave != 0;
  const uint32_t wt = MANY ? tid : tid - 64u;  // index among them (workers only)
  // Which points a thread owns.  One point per thread (!MANY): point blk x 448 + its index among the workers.  MANY: the
  // scan is dealt out in UNITS of 64 consecutive points (one wave's worth), every workgroup a contiguous run of
  // floor(U / grid) units and the first U mod grid workgroups one more, taken eight units (512 points) per pass —
  // so all workgroups hold the same number of points to within one unit.  (Dealing whole passes of grid x 512
  // points out instead left the last, partial pass to the first workgroups only: at C5 161 workgroups of 8 points
  // per thread and 95 of 7, 23 against 20 us to the barrier, and the round waits for the slowest.)
  uint32_t stride_pts = grid * W, first = worker ? blk * W + wt : n_pts, end_pts = n_pts;
  if constexpr (MANY) {
    const uint32_t units = (n_pts + 63u) / 64u, share = units / grid, extra = units % grid;  // uniform
    const uint32_t u0 = blk * share + (blk < extra ? blk : extra), u1 = u0 + share + (blk < extra ? 1u : 0u);
    stride_pts = W;
    first = u0 * 64u + wt;
    end_pts = u1 * 64u < n_pts ? u1 * 64u : n_pts;
  }
  const VoxelRecord* pay_base = a.dense ? a.dense : a.table;  // uniform: where a remembered record's payload is read from
  int4* memo = reinterpret_cast<int4*>(dyn_lds);
  double* stash = reinterpret_cast<double*>(dyn_lds + (size_t)a.memo_points * W * sizeof(int4));
  // parked points hold the planes that are read: 9 of a scan whose covariances are all bitwise symmetric, else 12
  const uint32_t park_planes = cov_sym ? 9u : (uint32_t)kScanPlanes;
  const uint32_t fit = a.stash_bytes / (park_planes * W * (uint32_t)sizeof(double));
  const uint32_t parked = MANY ? (fit < a.stash_points ? fit : a.stash_points) : 0u;  // uniform
  const bool folder = blk < (uint32_t)kFolders;  // folder g adds the rows of workgroups g, g + 16, g + 32 ...
  // row of workgroup b inside a buffer: the 16 rows of a folder are consecutive
  const uint32_t my_row = TEAM ? (blk % kFolders) * tv.folder_rows + blk / kFolders : (blk % kFolders) * kFolders + blk / kFolders;
  // rows of one buffer; TEAM: how many of a folder's 16 rows and of the 16 parts belong to a workgroup of the team
  const uint32_t buf_rows = TEAM ? (uint32_t)kFolders * tv.folder_rows : (uint32_t)kExchangeRows;
  const uint32_t live_rows = TEAM ? (tv.team_wgs - blk + (uint32_t)kFolders - 1u) / (uint32_t)kFolders : (uint32_t)kFolders;  // folders only
  const uint32_t live_parts = TEAM ? (tv.team_wgs < (uint32_t)kFolders ? tv.team_wgs : (uint32_t)kFolders) : (uint32_t)kFolders;

  Pose total;
#pragma unroll
  for (int k = 0; k < 9; ++k) total.R[k] = a.pose0[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) total.t[k] = a.pose0[9 + k];
  const double cos_thr = a.cosine_threshold, tsq_thr = a.translation_sq_threshold;
  const int max_it = a.max_iteration;
  const double inv_voxel = 1.0 / a.voxel_size;
  const double same_margin = 0x1p-20 * a.voxel_size;  // same_voxel_coord
  RobustSetting robust;
  if constexpr (ROBUST) robust = robust_setting(a.robust.kernel, a.robust.scale2, a.robust.gate);  // uniform

  double q0[kScanPlanes];
#pragma unroll
  for (int k = 0; k < kScanPlanes; ++k) q0[k] = 0.0;
  const bool have = first < end_pts;
  if constexpr (FUSED) {
    if (!fused_round0_load(up, a.stride, n_pts, reinterpret_cast<double*>(dyn_lds), &leave_sh, q0)) {
      if (tid == 0) a.state->abort_seq = a.seq;   // a unit never came: the host re-packs and re-runs the align
      return;
    }
  } else if (have) {
    load_point(a.scan, a.stride, first, q0);
  }

  // The look-ahead's keys name nothing when a launch starts — no memo survives a launch, the map may change in between —
  // so a launch's FIRST look-ahead takes every key as unknown and writes it.  That is round 0's; the fused align's is
  // round 1's, because its round-0 load holds the area through round 0.
  constexpr int kFirstLook = FUSED ? 1 : 0;

  // what the first point used last round: key, hit flag, voxel payload (raw)
  bool spec = false, hit = false;
  int32_t okx = 0, oky = 0, okz = 0;
  double mu[3] = {0.0, 0.0, 0.0}, Sv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Sv[k] = 0.0;

  uint64_t t_mark = STAMPS ? wall_clock64() : 0;
  uint64_t acc_body = 0, acc_l1 = 0, acc_l2 = 0, acc_solve = 0;
  uint64_t fine[4] = {0, 0, 0, 0};   // STAMPS: inside "solve + broadcast": totals to registers, LDL^T, exp + compose, publication
  bool conv_keep = false;            // wave 0: the last round's convergence verdict, for the final state
  int it = 0;
  bool gave_up = false;
  for (;;) {
    const double* R = total.R;
    const double* t = total.t;
    if (worker) {
      double v[kSlots];
#pragma unroll
      for (int k = 0; k < kSlots; ++k) v[k] = 0.0;
      if constexpr (!MANY) {
        if (have) {
          double p[3], C[9], S[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) C[k] = q0[3 + k];
          transform_point(R, t, q0[0], q0[1], q0[2], p);
          const int32_t kx = voxel_coord_fast(p[0], a.voxel_size, inv_voxel);
          const int32_t ky = voxel_coord_fast(p[1], a.voxel_size, inv_voxel);
          const int32_t kz = voxel_coord_fast(p[2], a.voxel_size, inv_voxel);
          if (!spec || kx != okx || ky != oky || kz != okz) {
            bool served = false;
            if (spec && prefetch && it > kFirstLook) {   // (nothing has been looked up before the first look-ahead)
              const int4 m = pf_key[tid - 64];
              if (m.x == kx && m.y == ky && m.z == kz && (uint32_t)m.w != kMemoNone) {
                served = true;
                hit = (uint32_t)m.w != kMemoMiss;
                if (hit) unpack_payload<kWorkers>(pf_pay + (tid - 64), mu, Sv);
              }
            }
            if (!served) hit = find_and_load(a.table, a.mask, kx, ky, kz, mu, Sv);
            okx = kx; oky = ky; okz = kz;
            spec = true;
          }
          if (hit) {
#pragma unroll
            for (int k = 0; k < 9; ++k) S[k] = Sv[k];
            accumulate_match<true, ROBUST>(R, p, C, mu, S, v, robust);
          }
        }
      } else {
        // one point: transform, key, the memo of point e (if it has one), accumulate
        auto one_point = [&](const double (&q)[kScanPlanes], uint32_t e, auto first_of_round) {
          double p[3], C[9], m2[3], S[9];
          transform_point(R, t, q[0], q[1], q[2], p);
          bool got;
          if (e < a.memo_points) {
            int4* mslot = memo + (size_t)e * W + wt;
            const int4 m = *mslot;
            // still inside last round's voxel?  (true implies an unchanged key; the key itself is made only otherwise)
            const bool stayed = ((int)(it != 0) & (int)same_voxel_coord(p[0], m.x, a.voxel_size, same_margin) &
                                 (int)same_voxel_coord(p[1], m.y, a.voxel_size, same_margin) &
                                 (int)same_voxel_coord(p[2], m.z, a.voxel_size, same_margin)) != 0;
            if (stayed) {
              got = (uint32_t)m.w != kMemoMiss;
              if (got) load_payload(pay_base + (uint32_t)m.w, m2, S);
            } else {
              const int32_t kx = voxel_coord_fast(p[0], a.voxel_size, inv_voxel);
              const int32_t ky = voxel_coord_fast(p[1], a.voxel_size, inv_voxel);
              const int32_t kz = voxel_coord_fast(p[2], a.voxel_size, inv_voxel);
              if (it != 0 && m.x == kx && m.y == ky && m.z == kz) {  // a point right below a face: key unchanged after all
                got = (uint32_t)m.w != kMemoMiss;
                if (got) load_payload(pay_base + (uint32_t)m.w, m2, S);
              } else {
                const VoxelRecord* rec = find_voxel(a.table, a.mask, kx, ky, kz);
                got = rec != nullptr;
                // what the memo remembers: the record's slot, or (dense copy in use) its index there, which the
                // compaction left in the upper half of the record's spare word — the same 128-byte line as the key
                uint32_t where = kMemoMiss;
                if (got) where = a.dense ? reinterpret_cast<const uint32_t*>(&rec->reserved)[1] : (uint32_t)(rec - a.table);
                *mslot = make_int4(kx, ky, kz, (int32_t)where);
                if (got) load_payload(rec, m2, S);
              }
            }
          } else {
            const int32_t kx = voxel_coord_fast(p[0], a.voxel_size, inv_voxel);
            const int32_t ky = voxel_coord_fast(p[1], a.voxel_size, inv_voxel);
            const int32_t kz = voxel_coord_fast(p[2], a.voxel_size, inv_voxel);
            got = find_and_load(a.table, a.mask, kx, ky, kz, m2, S);
          }
          if (got) {
#pragma unroll
            for (int k = 0; k < 9; ++k) C[k] = q[3 + k];
            accumulate_match<decltype(first_of_round)::value, ROBUST>(R, p, C, m2, S, v, robust);
          }
        };
        // the thread's first point stays in registers (its voxel record does not: the memo finds it), the next
        // a.stash_points are parked in LDS after round 0, the rest is re-read from HBM every round
        if (have) one_point(q0, 0u, Flag<true>{});
        uint32_t e = 1;
        for (uint32_t i = first + stride_pts; i < end_pts; i += stride_pts, ++e) {
          double q[kScanPlanes];
          if (e <= parked) {
            double* slot = stash + (size_t)(e - 1) * park_planes * W + wt;
            if (it == 0) {
              load_point_sym(a.scan, a.stride, i, q, cov_sym);
              if (cov_sym) {
                constexpr int kUsed[9] = {0, 1, 2, 3, 4, 5, 7, 8, 11};
#pragma unroll
                for (int j = 0; j < 9; ++j) slot[j * W] = q[kUsed[j]];
              } else {
#pragma unroll
                for (int k = 0; k < kScanPlanes; ++k) slot[k * W] = q[k];
              }
            } else if (cov_sym) {
              constexpr int kUsed[9] = {0, 1, 2, 3, 4, 5, 7, 8, 11};
#pragma unroll
              for (int j = 0; j < 9; ++j) q[kUsed[j]] = slot[j * W];
              q[6] = q[4]; q[9] = q[5]; q[10] = q[8];
            } else {
#pragma unroll
              for (int k = 0; k < kScanPlanes; ++k) q[k] = slot[k * W];
            }
          } else {
            load_point_sym(a.scan, a.stride, i, q, cov_sym);
          }
          one_point(q, e, Flag<false>{});
        }
      }
      wave_fold_to_lds(v, lane, red[wave]);
    }
    __syncthreads();
    if (STAMPS) { const uint64_t n = wall_clock64(); acc_body += n - t_mark; t_mark = n; }

    if (FUSED && it == 0) {
      // The fused align's round 0: the workgroup's row is on its way (wave 0 publishes it while the workers get here), so
      // the resident copy of its points leaves now, beside the exchange, instead of in front of the cold voxel probe.
      // The look-ahead, which writes the LDS the copy is read from, starts a round later (behind barrier 2).
      if (worker) fused_leave_resident(&leave_sh, reinterpret_cast<const double*>(dyn_lds), q0);
    } else if (!MANY && worker && prefetch && have) {
      // While wave 0 exchanges and solves: where is this point inside its voxel?  If a face is nearer than
      // prefetch_margin voxels, look the voxel behind it up now (full probe; 2 dependent round trips that
      // nobody waits for) so that next round's key change finds the record in LDS.  The map does not change during a
      // launch: a neighbour that pf_key already names (looked up in an earlier round of THIS launch — the launch's first
      // look-ahead, kFirstLook, takes no key as known) is not probed again, its record is still what the table holds.
      double p[3], rx, ry, rz;  // r*: distance of the point from the lower face of its voxel, in [0, voxel)
      transform_point(R, t, q0[0], q0[1], q0[2], p);
      (void)voxel_coord_fast(p[0], a.voxel_size, inv_voxel, &rx);
      (void)voxel_coord_fast(p[1], a.voxel_size, inv_voxel, &ry);
      (void)voxel_coord_fast(p[2], a.voxel_size, inv_voxel, &rz);
      const double half = 0.5 * a.voxel_size;
      const double dx = fmin(rx, a.voxel_size - rx), dy = fmin(ry, a.voxel_size - ry), dz = fmin(rz, a.voxel_size - rz);
      int32_t nx = okx, ny = oky, nz = okz;
      double d;
      if (dx <= dy && dx <= dz) { d = dx; nx += rx < half ? -1 : 1; }
      else if (dy <= dz) { d = dy; ny += ry < half ? -1 : 1; }
      else { d = dz; nz += rz < half ? -1 : 1; }
      const int4 known = pf_key[tid - 64];
      if (it == kFirstLook || known.x != nx || known.y != ny || known.z != nz || (uint32_t)known.w == kMemoNone) {
        int4 m = make_int4(nx, ny, nz, (int32_t)kMemoNone);
        if (d < a.prefetch_margin * a.voxel_size) {
          const VoxelRecord* rec = find_voxel(a.table, a.mask, nx, ny, nz);
          m.w = rec ? (int32_t)(uint32_t)(rec - a.table) : (int32_t)kMemoMiss;
          if (rec) {
            const double2* pay = reinterpret_cast<const double2*>(rec->mean);
            double2* dst = pf_pay + (tid - 64);
#pragma unroll
            for (int j = 0; j < 6; ++j) dst[j * kWorkers] = pay[j];
          }
        }
        pf_key[tid - 64] = m;
      }
    }
    // STAMPS: how long the look-ahead kept this wave (reported in the worker lane's "level-1" column)
    if (STAMPS && !MANY && wave != 0) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const uint64_t n = wall_clock64(); acc_l1 += n - t_mark; t_mark = n; }

    if (wave == 0) {
      // Addresses that depend on the lane are re-made here every round: hoisted out of the loop they would sit in
      // registers through the whole accumulate phase (the MANY instantiations spilled them to scratch).
      uint32_t lane_here = tid & 63;
      asm volatile("" : "+v"(lane_here));
      const uint32_t lane = lane_here;
      // the buffers rotate with a round number that runs on from launch to launch (a.round0: rounds executed on
      // this context before): nothing has to be tidied up when a launch ends
      const uint32_t buf = (a.round0 + (uint32_t)it) % 3u;
      double* rows = a.rows + (size_t)buf * buf_rows * kSlots;
      double* parts = a.parts + (size_t)buf * kFolders * kSlots;
      // ---- level 1: publish this workgroup's row (every re-arming store of mine has completed) ----
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane <= (uint32_t)kCountSlot) {
        double w_sum[kWaves];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) w_sum[w] = red[w][lane];
        const double row_sum = MANY ? tree_sum<kWaves>(w_sum) : tree_sum<kWaves - 1>(w_sum + 1);
        store_through_bits(rows + (size_t)my_row * kSlots + lane, publishable(row_sum));
      }
      bool ok = true;
      // the fused align's round 0: some workgroups publish a whole upload before the last one has its points
      const uint32_t spin_limit = (FUSED && it == 0 && up.spin_limit > a.spin_limit) ? up.spin_limit : a.spin_limit;
      if (folder) {  // uniform
        double part = 0.0;
        if constexpr (TEAM) ok = poll_and_sum<false, true>(rows + (size_t)blk * tv.folder_rows * kSlots, lane, spin_limit, part, live_rows);
        else ok = poll_and_sum<false>(rows + (size_t)blk * kFolders * kSlots, lane, spin_limit, part);
        if (ok && lane <= (uint32_t)kCountSlot) store_through_bits(parts + (size_t)blk * kSlots + lane, publishable(part));
      }
      if (STAMPS) { const uint64_t n = wall_clock64(); acc_l1 += n - t_mark; t_mark = n; }
      // ---- level 2: every workgroup adds the parts ----
      double tot = 0.0;
      if (!MULTI) {
        // A workgroup that is no folder has nothing to find before the folders have gathered their rows (a hop of
        // ~1.5 us): polling the parts from the start only puts 240 workgroups' loads into the queues the 16 folders'
        // polls and stores go through.  One point per thread (C2): 6.82 -> 6.55 us per round with 64 units (50: 6.63,
        // 60 - 70: 6.55, 85: 6.9, 100: 7.1); several points per thread (C5): no gain, not delayed.
        if (!MANY && !folder) __builtin_amdgcn_s_sleep(kL2Delay);
        if constexpr (TEAM) { if (ok) ok = poll_and_sum<false, true>(parts, lane, spin_limit, tot, live_parts); }
        else if (ok) ok = poll_and_sum<false>(parts, lane, spin_limit, tot);
      } else {
        // ---- several GPUs: workgroup 0 adds the parts to this rank's total and stores it into the mailbox
        // of every rank (its own included); every workgroup then adds the ranks' totals in rank order ----
        const uint32_t mbuf = (a.mail_round0 + (uint32_t)it) % 3u;
        if (blk == 0) {
          double mine = 0.0;
          if (ok) ok = poll_and_sum<false>(parts, lane, a.spin_limit, mine);
          if (ok && lane <= (uint32_t)kCountSlot) {
            const unsigned long long bits = publishable(mine);
            for (uint32_t r = 0; r < a.world; ++r)
              store_system_bits(a.mail[r] + ((size_t)mbuf * kMaxRanks + a.rank) * kSlots + lane, bits);
          }
        }
        if (ok) ok = poll_and_sum<true>(a.mail[a.rank] + (size_t)mbuf * kMaxRanks * kSlots, lane, a.spin_limit, tot);
        // (the mailbox buffer everyone finished with a round ago is re-armed behind the round's last barrier, with the
        // rows and parts)
      }
      if (STAMPS) { const uint64_t n = wall_clock64(); acc_l2 += n - t_mark; t_mark = n; }
      if (!ok) {
        if (lane == 0) stop_sh = 2;
      } else {
        // (what was consumed a round ago is re-armed, and the round's row of the log written, BEHIND the barrier below:
        // a release fence — the one in front of the LDS hand-over here, the one inside __syncthreads — makes the wave
        // wait for every store it has in flight, and a write-through store takes its time; this wave's part of the
        // round is the one everybody waits for)
        if (lane < kSlots) totals[lane] = lane <= (uint32_t)kCountSlot ? tot : 0.0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const double* solve = totals;   // PRIOR: the log's row (behind the barrier below) stays the data sums
        if constexpr (PRIOR) solve = prior_solve_totals(a, total, totals, lane);
        double A[21], g[6], xi[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) A[k] = solve[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = -solve[21 + k];
        uint64_t f0 = 0, f1 = 0, f2 = 0;
        if (STAMPS) { f0 = pinned_clock(A); fine[0] += f0 - t_mark; }
        if (!ldlt6_solve_spd(A, g, xi)) ldlt6_solve_pivoted(solve, work, lane, xi);  // uniform branch
        if (STAMPS) { f1 = pinned_clock(xi); fine[1] += f1 - f0; }
        Pose next, step;
        se3_exp_device(xi, step);
        pose_compose(step, total, next);
        conv_keep = converged(step, cos_thr, tsq_thr);
        if (STAMPS) { f2 = pinned_clock(next.R); fine[2] += f2 - f1; }
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < 9; ++k) pose_sh[k] = next.R[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) pose_sh[9 + k] = next.t[k];
          stop_sh = (conv_keep || (it + 1 >= max_it)) ? 1 : 0;
        }
        if (STAMPS) fine[3] += wall_clock64() - f2;
      }
    }
    __syncthreads();
    const int stop = stop_sh;
    if (stop == 2) { gave_up = true; break; }  // uniform: a workgroup never published (not all resident?)
    if (wave == 0) {
      // Off the round's critical path (the other waves are already transforming their points with the new pose): re-arm
      // what was consumed a round ago.  In a launch's first round that is what the launch BEFORE published last:
      // everyone has published this round, so everyone has left that launch and its reads behind.  (Before the very
      // first round of a context the buffer is unset already; storing "unset" again is harmless.)  The stores are
      // complete long before this wave publishes again (s_waitcnt vmcnt(0) in front of the publication).
      uint32_t lane_here = tid & 63;
      asm volatile("" : "+v"(lane_here));
      const uint32_t rearm = (a.round0 + (uint32_t)it + 2u) % 3u;
      if (lane_here <= (uint32_t)kCountSlot) {
        store_through_bits(a.rows + ((size_t)rearm * buf_rows + my_row) * kSlots + lane_here, kRowUnset);
        if (folder) store_through_bits(a.parts + ((size_t)rearm * kFolders + blk) * kSlots + lane_here, kRowUnset);
      }
      if (MULTI && blk == 0 && lane_here <= (uint32_t)kCountSlot) {
        // ... and the mailbox buffer everyone (on every rank) finished with a round ago; the running round number
        // carries over from launch to launch, so there is no clean-up at the end of a launch
        const uint32_t old = (a.mail_round0 + (uint32_t)it + 2u) % 3u;
        for (uint32_t r = 0; r < a.world; ++r)
          store_system_bits(a.mail[a.rank] + ((size_t)old * kMaxRanks + r) * kSlots + lane_here, kRowUnset);
      }
      // the round's row of the log: still in LDS (written again only after the next round's barrier)
      if (blk == 0 && lane_here < kSlots) a.log[(size_t)it * kSlots + lane_here] = totals[lane_here];
    }
    load_pose(pose_sh, total);
    ++it;
    if (STAMPS) { const uint64_t n = wall_clock64(); acc_solve += n - t_mark; t_mark = n; }
    if (stop) break;
  }
  if (gave_up) {
    // The host sees state->seq != seq (workgroup 0) or state->abort_seq == seq (any other workgroup: it may have
    // timed out although workgroup 0 found everything in place), resets the exchange buffers and uses launches.
    if (tid == 0) { if constexpr (TEAM) *tv.abort_word = a.seq; else a.state->abort_seq = a.seq; }
    if (MULTI && blk == 0 && tid < a.world)   // the peers learn it from the verdict word, at the latest at their end
      store_system_bits(a.mail[tid] + kMailRowWords + a.rank, (unsigned long long)a.mail_seq << 1);
    return;
  }

  if (wave == 0 && blk == 0) {
    uint32_t outcome = kOutcomeCommitted;
    if (MULTI) {
      // All ranks commit this align or none does: every rank's workgroup 0 tells every rank how its loop ended and
      // waits for everybody's word.  (A rank that gave up alone would otherwise re-run the align through the host
      // collective while a late peer, finding that rank's last row already in its mailbox, returns success.)
      const unsigned long long mine = ((unsigned long long)a.mail_seq << 1) | 1ull;
      if (lane < a.world) store_system_bits(a.mail[lane] + kMailRowWords + a.rank, mine);
      const double* src = a.mail[a.rank] + kMailRowWords + (lane < a.world ? lane : 0u);
      unsigned long long w = lane < a.world ? load_system_bits(src) : mine;
      bool late = false;
      for (uint32_t spins = 0; __any((w >> 1) < a.mail_seq); ++spins) {
        if (spins >= a.spin_limit) { late = true; break; }
        __builtin_amdgcn_s_sleep(1);
        if ((w >> 1) < a.mail_seq) w = load_system_bits(src);
      }
      if (late) outcome = kOutcomeNoAgreement;
      else if (__any(w != mine)) outcome = kOutcomeAgreedAbort;
    }
    if (lane == 0) {
      AlignState* out = a.state;
      out->outcome = outcome;
      if (outcome == kOutcomeCommitted) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out->pose[k] = total.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) out->pose[9 + k] = total.t[k];
        out->cosine_threshold = cos_thr;
        out->translation_sq_threshold = tsq_thr;
        out->max_iteration = max_it;
        out->iteration = it;
        out->converged = conv_keep ? 1 : 0;   // (the last increment itself, AlignState::step, is not reported by this launch)
        out->done = 1;
        out->pad = 0;
        if constexpr (FUSED)
          out->unit_to_end_ticks = wall_clock64() - __hip_atomic_load(up.unit_clock, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out->seq = a.seq;
      }
    }
  }
  if (STAMPS && tid == 0) atomicAdd((unsigned long long*)&a.stamps[32 + blk], (unsigned long long)acc_body);
  if (STAMPS && blk == 0 && (tid == 0 || tid == 64)) {
    const int o = tid == 0 ? 8 : 16;  // solver wave / first worker lane
    atomicAdd((unsigned long long*)&a.stamps[o + 0], (unsigned long long)acc_body);
    atomicAdd((unsigned long long*)&a.stamps[o + 1], (unsigned long long)acc_l1);
    atomicAdd((unsigned long long*)&a.stamps[o + 2], (unsigned long long)acc_l2);
    atomicAdd((unsigned long long*)&a.stamps[o + 3], (unsigned long long)acc_solve);
    atomicAdd((unsigned long long*)&a.stamps[o + 5], (unsigned long long)it);
    if (tid == 0)
      for (int k = 0; k < 4; ++k) atomicAdd((unsigned long long*)&a.stamps[24 + k], (unsigned long long)fine[k]);
  }
}

// The launch.  A MANY launch is planned from a.n, which is an UPPER BOUND for a scan whose size is still on the device
// (a scan prepared there and aligned without waiting for its count): when the real size turns out to fit the grid
// after all, the workgroups run the one-point-per-thread body — the mapping, the sums and hence the bits of the launch
// that a settled scan of that size gets (without the neighbour prefetch, which changes no result) — so the chain that
// does not wait returns the bits of the one that does, whatever the sweep's raw size.
template <int BLOCK, bool MULTI, bool STAMPS, bool MANY, bool ROBUST = false, bool PRIOR = false>
__global__ __launch_bounds__(BLOCK) void persistent_kernel(PersistArgs a) {
  const FusedUpload none{};
  if constexpr (MANY) {
    const uint32_t n_pts = a.n_dev ? (*a.n_dev < a.n ? *a.n_dev : a.n) : a.n;  // uniform
    if (n_pts <= gridDim.x * (uint32_t)(BLOCK - 64)) {
      persistent_body<BLOCK, MULTI, STAMPS, false, false, false, ROBUST, PRIOR>(a, none);
      return;
    }
  }
  persistent_body<BLOCK, MULTI, STAMPS, MANY, false, false, ROBUST, PRIOR>(a, none);
}

// The fused align: the upload's packing happens inside round 0 (a separate kernel, so that the production
// instantiations above keep their code).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void persistent_fused_kernel(PersistArgs a, FusedUpload up) {
  persistent_body<BLOCK, false, false, false, true>(a, up);
}

// The batched align: team h = workgroups [h T, (h + 1) T) runs hypothesis h (TeamArgs in vgicp_device.h).  A kernel of
// its own, so that the instantiations above keep their code and their registers.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void persistent_team_kernel(PersistArgs a, TeamArgs t) {
  const uint32_t h = blockIdx.x / t.team_wgs;  // uniform
  if (h >= t.teams) return;
  const FusedUpload none{};
  TeamView tv;
  tv.vb = blockIdx.x - h * t.team_wgs;
  tv.team_wgs = t.team_wgs;
  tv.folder_rows = t.folder_rows;
  tv.abort_word = t.abort_word;
  a.rows += (size_t)h * 3 * kFolders * t.folder_rows * kSlots;
  a.parts += (size_t)h * 3 * kFolders * kSlots;
  a.state = reinterpret_cast<AlignState*>(reinterpret_cast<double*>(a.state) + (size_t)h * t.slot_words);
  a.log += (size_t)h * t.slot_words;
#pragma unroll
  for (int k = 0; k < 12; ++k) a.pose0[k] = t.pose0[h][k];
  persistent_body<BLOCK, false, false, false, false, true>(a, none, tv);
}

// Multi-GPU only: fold this rank's rows into one row (fixed order) so the all-reduce moves 256 B.
__global__ __launch_bounds__(1024) void fold_rows_kernel(const double* __restrict__ rows,
                                                         uint32_t nrows, const AlignState* state,
                                                         double* __restrict__ sums) {
  constexpr int kGroups = 1024 / kSlots;
  __shared__ double fin[kGroups][kSlots];
  if (state->done) return;  // rows are stale once the loop has ended; the value is never used
  const uint32_t tid = threadIdx.x, slot = tid & (kSlots - 1), group = tid / kSlots;
  double s = 0.0;
  for (uint32_t b = group; b < nrows; b += kGroups) s += rows[(size_t)b * kSlots + slot];
  fin[group][slot] = s;
  __syncthreads();
  if (tid < kSlots) {
    double tot = fin[0][tid];
#pragma unroll
    for (int g = 1; g < kGroups; ++g) tot += fin[g][tid];
    sums[tid] = tot;
  }
}

// out[o] = in[perm[o]] for the AoS arrays of a scan (points 3, covariances 9, optionally the input indices): the
// reordering of VGICP_OPTION_REFERENCE_ORDER (one thread per kept point; the planes are re-made by pack_scan_kernel).
__global__ void gather_scan_kernel(const uint32_t* __restrict__ perm, uint32_t m, const double* __restrict__ pts,
                                   const double* __restrict__ covs, const unsigned long long* __restrict__ idx,
                                   double* __restrict__ out_pts, double* __restrict__ out_covs,
                                   unsigned long long* __restrict__ out_idx) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= m) return;
  const uint32_t from = perm[o];
#pragma unroll
  for (int k = 0; k < 3; ++k) out_pts[3 * (size_t)o + k] = pts[3 * (size_t)from + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) out_covs[9 * (size_t)o + k] = covs[9 * (size_t)from + k];
  if (idx) out_idx[o] = idx[from];
}

// AoS (the caller's Eigen memory) -> 12 SoA planes.
__global__ void pack_scan_kernel(const double* __restrict__ pts, const double* __restrict__ covs,
                                 uint32_t n, double* __restrict__ soa, uint64_t stride, uint32_t* asym, uint32_t seq) {
  // *asym = seq as soon as one covariance is not bitwise symmetric (the word needs no clearing: seq differs per upload)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) soa[k * stride + i] = pts[3 * (size_t)i + k];
  double c[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    c[k] = covs[9 * (size_t)i + k];
    soa[(3 + k) * stride + i] = c[k];
  }
  const bool same = __double_as_longlong(c[1]) == __double_as_longlong(c[3]) &&
                    __double_as_longlong(c[2]) == __double_as_longlong(c[6]) &&
                    __double_as_longlong(c[5]) == __double_as_longlong(c[7]);
  if (!same) *asym = seq;
}

// The same packing for a scan that is still ARRIVING in page-locked host memory: the upload of vgicp_align /
// vgicp_scan_upload without the runtime's copy engine.  Host threads (plain copies, no HIP call: CopyCrew,
// vgicp_context.h) fill `apts` (n x 24 B) and `acov` in units of `unit` points and publish each unit by storing `seq`
// into flags[16 * u] (one 64-byte line per flag, written after the unit's bytes).  This ONE launch reads the staging
// memory over PCIe itself — 16-byte loads of consecutive lanes, a block's bytes through LDS — while the threads are
// still copying the units behind (tools/micro/stage_crew_probe.hip: a kernel gets 54 GB/s out of the link; staging +
// copy commands + pack took 0.45 ms).
// Round 6: the link is what bounds the upload, so a unit whose covariances are ALL bitwise symmetric — every covariance
// the reference produces is (src/CloudPreprocessor.cpp:119-123 apart from its indefinite corner) — crosses
// it as six doubles per point (c00 c10 c20 c11 c21 c22: 48 instead of 72 bytes, 72 instead of 96 per point in all), and
// the three mirrored entries are made here.  The host thread that copies a unit checks every covariance while it reads
// it anyway and says which form it wrote in flags[16 * u + 1] (kArenaCompact / kArenaFull, stored before the flag); a
// unit with ONE asymmetric covariance travels whole.  A unit's covariances start at acov + 72 * (first point) in both
// forms.  What lands on the device is the caller's scan bit for bit either way.
// Every block also leaves the AoS copy on the device (map insertion and download read it) and reports an asymmetric
// covariance like pack_scan_kernel.  wait == 0: everything is there already (the forms are still read from the flags).
// A wait that exceeds spin_limit polls (each a PCIe round trip, >= 1 us) ends the block's workgroup: the host, which
// knows how long its copy threads took, then repeats the packing without waiting behind this launch.
constexpr int kPackArenaBlock = 256;
__global__ __launch_bounds__(kPackArenaBlock) void pack_arena_kernel(
    const char* __restrict__ apts, const char* __restrict__ acov, uint32_t n, uint32_t unit, const uint32_t* flags,
    uint32_t wait, uint32_t seq, uint32_t spin_limit, double* __restrict__ aos_pts, double* __restrict__ aos_cov,
    double* __restrict__ soa, uint64_t stride, uint32_t* asym) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  constexpr uint32_t B = kPackArenaBlock;
  __shared__ __attribute__((aligned(16))) double lds[12 * B];
  __shared__ __attribute__((aligned(16))) double lds_compact[6 * B];
  __shared__ uint32_t ok, form_sh;
  const uint32_t t = threadIdx.x, blocks = (n + B - 1) / B;
  uint32_t have_unit = 0xFFFFFFFFu;
  for (uint32_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    const uint32_t p0 = b * B, cnt = min(B, n - p0);
    const uint32_t u = p0 / unit;   // unit is a multiple of the block: a block never straddles two units
    if (u != have_unit) {
      if (t == 0) {
        uint32_t good = 1;
        unsigned long long w = load_flag_and_form(flags, u);   // flag and form in one load over the link
        if (wait)
          for (uint32_t spins = 0; (uint32_t)w != seq; ++spins) {
            if (spins >= spin_limit) { good = 0; break; }
            __builtin_amdgcn_s_sleep(20);
            w = load_flag_and_form(flags, u);
          }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        ok = good;
        form_sh = good ? (uint32_t)(w >> 32) : kArenaFull;
      }
      __syncthreads();
      if (!ok) return;   // uniform
      have_unit = u;
    }
    const bool compact = form_sh == kArenaCompact;   // uniform
    const v4i* sp = reinterpret_cast<const v4i*>(apts + (size_t)p0 * 24);
    v4i* lp = reinterpret_cast<v4i*>(lds);
    v4i* lc = reinterpret_cast<v4i*>(lds + 3 * B);
    // an odd count (the scan's last block only) leaves half a 16-byte chunk at the end of the points AND of the full
    // covariances: read whole (the staging areas are padded), stored to the device copy as 8 bytes
    const uint32_t np = (cnt * 24 + 15) / 16, np_whole = (cnt * 24) / 16, nc = (cnt * 72 + 15) / 16, nc_whole = (cnt * 72) / 16;
    v4i* dp = reinterpret_cast<v4i*>(aos_pts + 3 * (size_t)p0);
    v4i* dc = reinterpret_cast<v4i*>(aos_cov + 9 * (size_t)p0);
    for (uint32_t k = t; k < np; k += B) {
      const v4i w = __builtin_nontemporal_load(sp + k);
      lp[k] = w;
      if (k < np_whole) dp[k] = w;
    }
    if (!compact) {
      const v4i* sc = reinterpret_cast<const v4i*>(acov + (size_t)p0 * 72);
      for (uint32_t k = t; k < nc; k += B) {
        const v4i w = __builtin_nontemporal_load(sc + k);
        lc[k] = w;
        if (k < nc_whole) dc[k] = w;
      }
    } else {
      // the unit's compact records are contiguous from the unit's start: this block's begin (p0 - unit start) * 48 in
      const uint32_t u0 = u * unit;
      const v4i* sc = reinterpret_cast<const v4i*>(acov + (size_t)u0 * 72 + (size_t)(p0 - u0) * 48);
      v4i* lq = reinterpret_cast<v4i*>(lds_compact);
      for (uint32_t k = t; k < cnt * 3; k += B) lq[k] = __builtin_nontemporal_load(sc + k);   // 48 B = three chunks per point
    }
    __syncthreads();
    if (t == 0 && np != np_whole) {
      aos_pts[3 * (size_t)(p0 + cnt) - 1] = lds[3 * cnt - 1];
      if (!compact) aos_cov[9 * (size_t)(p0 + cnt) - 1] = lds[3 * B + 9 * cnt - 1];
    }
    if (t < cnt) {
      const size_t i = p0 + t;
#pragma unroll
      for (int k = 0; k < 3; ++k) soa[k * stride + i] = lds[3 * t + k];
      double c[9];
      if (compact) {
        const double a0 = lds_compact[6 * t], a1 = lds_compact[6 * t + 1], a2 = lds_compact[6 * t + 2],
                     a3 = lds_compact[6 * t + 3], a4 = lds_compact[6 * t + 4], a5 = lds_compact[6 * t + 5];
        c[0] = a0; c[1] = a1; c[2] = a2; c[3] = a1; c[4] = a3; c[5] = a4; c[6] = a2; c[7] = a4; c[8] = a5;
#pragma unroll
        for (int k = 0; k < 9; ++k) lds[3 * B + 9 * t + k] = c[k];   // the whole record for the device copy below
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) c[k] = lds[3 * B + 9 * t + k];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) soa[(3 + k) * stride + i] = c[k];
      const bool same = __double_as_longlong(c[1]) == __double_as_longlong(c[3]) &&
                        __double_as_longlong(c[2]) == __double_as_longlong(c[6]) &&
                        __double_as_longlong(c[5]) == __double_as_longlong(c[7]);
      if (!same) *asym = seq;
    }
    __syncthreads();
    if (compact) {   // the device's AoS copy of the covariances, whole records, coalesced out of LDS
      const uint32_t words = cnt * 9;   // doubles
      for (uint32_t k = t; k < words / 2; k += B) dc[k] = lc[k];
      if (t == 0 && (words & 1u)) aos_cov[9 * (size_t)p0 + words - 1] = lds[3 * B + words - 1];
      __syncthreads();
    }
  }
}

}  // namespace

// ---- the round kernels' instantiations: one table of kernel pointers per list of vgicp_launch_plan.h, built from the
// list itself, so that what exists, what has its LDS limit raised and what a plan can pick are one set ----
namespace {
using IterateFn = void (*)(IterArgs);
using PersistentFn = void (*)(PersistArgs);
template <size_t... I>
constexpr std::array<IterateFn, sizeof...(I)> iterate_table(std::index_sequence<I...>) {
  return {{&iterate_kernel<kIterateVariants[I].block, kIterateVariants[I].robust, kIterateVariants[I].prior>...}};
}
template <size_t... I>
constexpr std::array<IterateFn, sizeof...(I)> close_table(std::index_sequence<I...>) {
  return {{&close_kernel<kCloseVariants[I].block, kCloseVariants[I].prior>...}};
}
template <size_t... I>
constexpr std::array<PersistentFn, sizeof...(I)> persistent_table(std::index_sequence<I...>) {
  return {{&persistent_kernel<512, kPersistentVariants[I].multi, kPersistentVariants[I].stamps, kPersistentVariants[I].many,
                              kPersistentVariants[I].robust, kPersistentVariants[I].prior>...}};
}
constexpr auto kIterateKernels = iterate_table(std::make_index_sequence<kIterateVariantCount>{});
constexpr auto kCloseKernels = close_table(std::make_index_sequence<kCloseVariantCount>{});
constexpr auto kPersistentKernels = persistent_table(std::make_index_sequence<kPersistentVariantCount>{});
}  // namespace

hipError_t launch_iterate(hipStream_t s, const IterArgs& args, uint32_t grid, int block) {
  const int v = plan_iterate(block, args.robust.kernel, args.robust.gate, args.prior.on != 0);
  if (v == kLaunchRefused) return hipErrorInvalidValue;
  counted_launch(kIterateKernels[v], dim3(grid), dim3(block), 0, s, args);
  return hipGetLastError();
}

namespace {
// kPersistWorkers, kPersistWide, kMemoBytesPerPoint, kPersistDynLds, kPrefetchBytes: vgicp_launch_plan.h
static_assert(kMemoBytesPerPoint == kPersistWide * sizeof(int4) &&
              kPrefetchBytes == kPersistWorkers * (sizeof(int4) + 6 * sizeof(double2)), "the plan's LDS sizes are the kernel's");
constexpr uint32_t kMaxMemoPoints = 12;  // beyond that a thread's points are looked up every round
constexpr uint32_t kFusedLoadBytes = kPersistWorkers * 18 * sizeof(double);  // fused_round0_load: 64 512
}  // namespace

// The plan is made from n, which may be an upper bound of the scan's size (a scan prepared on the device): it is
// sized for 512 point-carrying threads; a launch that finds fewer points than grid x 448 uses 448 and less of it.
void persistent_lds_plan(uint32_t n, uint32_t grid, uint32_t* memo_points, uint32_t* stash_points, uint32_t* stash_bytes,
                         uint32_t lds_budget) {
  *memo_points = *stash_points = *stash_bytes = 0;
  // lds_budget: 0 = the whole CU (kPersistDynLds); contexts that SHARE a device take less, so that two of their
  // workgroups fit one CU (what is not kept in LDS is re-read: same arithmetic, same bits)
  const uint32_t budget = (lds_budget == 0 || lds_budget > kPersistDynLds) ? kPersistDynLds : lds_budget;
  if ((uint64_t)n <= (uint64_t)grid * kPersistWorkers) return;  // one point per thread: registers (and the neighbour prefetch area)
  // units of 64 points, dealt out evenly: a workgroup holds at most ceil(units / grid), taken 8 units per pass
  const uint32_t units = (n + 63u) / 64u, most = (units + grid - 1) / grid;
  const uint32_t per_thread = (most + kPersistWide / 64 - 1) / (kPersistWide / 64);  // points per thread (upper bound)
  // the memo first (it saves the table access, the larger term), the rest of the LDS parks whole points
  uint32_t memo = per_thread < kMaxMemoPoints ? per_thread : kMaxMemoPoints;
  if (memo * kMemoBytesPerPoint > budget) memo = budget / kMemoBytesPerPoint;
  *memo_points = memo;
  *stash_points = per_thread - 1;  // the first point of a thread lives in registers
  *stash_bytes = *stash_points ? budget - memo * kMemoBytesPerPoint : 0u;
}

size_t persistent_rows_words() { return 3 * (size_t)kExchangeRows * kSlots; }
size_t persistent_parts_words() { return 3 * (size_t)kFolders * kSlots; }

// Initial / between-launch content of the exchange buffers for a launch of `grid` workgroups: the words a
// workgroup (rows) or a folder (parts) publishes are unset, every other word is +0.0 for good, so that
// every folder adds 16 rows and every workgroup adds 16 parts whatever the grid.
void persistent_exchange_image(uint32_t grid, unsigned long long* rows_words, unsigned long long* parts_words) {
  for (int buf = 0; buf < 3; ++buf) {
    unsigned long long* rw = rows_words + (size_t)buf * kExchangeRows * kSlots;
    for (size_t w = 0; w < (size_t)kExchangeRows * kSlots; ++w) rw[w] = 0ull;
    for (uint32_t b = 0; b < grid && b < (uint32_t)kExchangeRows; ++b) {
      const uint32_t row = (b % kFolders) * kFolders + b / kFolders;
      for (int sl = 0; sl <= kCountSlot; ++sl) rw[(size_t)row * kSlots + sl] = kRowUnset;
    }
    unsigned long long* pw = parts_words + (size_t)buf * kFolders * kSlots;
    for (size_t w = 0; w < (size_t)kFolders * kSlots; ++w) pw[w] = 0ull;
    for (uint32_t g = 0; g < grid && g < (uint32_t)kFolders; ++g)
      for (int sl = 0; sl <= kCountSlot; ++sl) pw[(size_t)g * kSlots + sl] = kRowUnset;
  }
}

// LDS beyond the default 64 KB per workgroup has to be asked for, per device and per instantiation.  Done when a
// context is created, NOT at the first launch: the launch path of a persistent kernel must not contain a runtime
// call that may wait for the device — with several sub-contexts on one device another sub-context's launch is
// already running (and waiting for this one) by then.
hipError_t persistent_prepare_device() {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&persistent_fused_kernel<512>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPersistDynLds);
  for (PersistentFn fn : kPersistentKernels)
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPersistDynLds);
  return e;
}

hipError_t launch_persistent(hipStream_t s, const PersistArgs& args, uint32_t grid) {
  PersistentFacts f;
  f.world = args.world;
  f.stamps = args.stamps != nullptr;
  f.n = args.n;
  f.grid = grid;
  f.memo_points = args.memo_points;
  f.stash_bytes = args.stash_bytes;
  f.prefetch_margin = args.prefetch_margin;
  f.robust_kernel = args.robust.kernel;
  f.robust_gate = args.robust.gate;
  f.prior = args.prior.on != 0;
  const PersistentPlan plan = plan_persistent(f);
  if (plan.variant == kLaunchRefused) return hipErrorInvalidValue;
  counted_launch(kPersistentKernels[plan.variant], dim3(grid), dim3(512), plan.dyn_lds, s, args);
  return hipGetLastError();
}

hipError_t launch_persistent_fused(hipStream_t s, const PersistArgs& args, const FusedUpload& up, uint32_t grid) {
  // one point per thread only: no memo, no stash; the round-0 load borrows the neighbour-prefetch area
  if (args.memo_points != 0 || args.stash_bytes != 0 || args.world > 1 || args.stamps != nullptr || args.n_dev != nullptr ||
      (uint64_t)args.n > (uint64_t)grid * kPersistWorkers || up.unit < kPersistWorkers)
    return hipErrorInvalidValue;
  const size_t dyn = std::max<size_t>(args.prefetch_margin > 0.0 ? kPrefetchBytes : 0u, kFusedLoadBytes);
  counted_launch(persistent_fused_kernel<512>, dim3(grid), dim3(512), dyn, s, args, up);
  return hipGetLastError();
}

hipError_t launch_persistent_teams(hipStream_t s, const PersistArgs& args, const TeamArgs& teams, uint32_t grid) {
  // one point per thread, a settled scan, every team inside the grid and inside the exchange storage
  if (args.memo_points != 0 || args.stash_bytes != 0 || args.world > 1 || args.stamps != nullptr || args.n_dev != nullptr ||
      args.round0 != 0 || teams.teams < 1 || teams.teams > (uint32_t)kTeamsMax || teams.team_wgs < 1 ||
      (uint64_t)teams.teams * teams.team_wgs > grid || (uint64_t)args.n > (uint64_t)teams.team_wgs * kPersistWorkers ||
      teams.folder_rows != (teams.team_wgs + kFolders - 1) / kFolders ||
      (uint64_t)teams.teams * kFolders * teams.folder_rows > (uint64_t)kTeamRowsMax || teams.abort_word == nullptr)
    return hipErrorInvalidValue;
  const size_t dyn = args.prefetch_margin > 0.0 ? kPrefetchBytes : 0u;
  counted_launch(persistent_team_kernel<512>, dim3(grid), dim3(512), dyn, s, args, teams);
  return hipGetLastError();
}

// Whether `grid` 512-thread workgroups of the persistent kernel with this much dynamic LDS can all be
// resident at once on the current device (the in-kernel exchange requires it).
hipError_t persistent_max_resident(uint32_t dyn_lds_bytes, int cu_count, uint32_t* max_grid) {
  // the plain kernel with the most registers, the robust round's and the pose prior's (bodies of their own: asked on
  // their own)
  constexpr int asked[3] = {find_persistent(true, false, true, false, false), find_persistent(false, false, true, true, false),
                            find_persistent(false, false, true, true, true)};
  static_assert(asked[0] >= 0 && asked[1] >= 0 && asked[2] >= 0, "the three instantiations are listed");
  *max_grid = (uint32_t)cu_count;  // one workgroup per CU is what the design uses
  for (const int v : asked) {
    const void* fn = reinterpret_cast<const void*>(kPersistentKernels[v]);
    int per_cu = 0;
    // more than the default 64 KB of LDS per workgroup has to be asked for before the occupancy query can say yes
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPersistDynLds);
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 512, dyn_lds_bytes);
    if (e != hipSuccess) return e;
    if (per_cu <= 0) *max_grid = 0u;
  }
  return hipSuccess;
}

// The closing launch folds the last round's rows with the workgroup size of the body launches, so that
// its sums are added in the same order as every other round's (and as the persistent launch adds them).
hipError_t launch_close(hipStream_t s, const IterArgs& args, int block) {
  const int v = plan_close(block, args.prior.on != 0);   // the last round's solve takes the pose prior as every other round's
  if (v == kLaunchRefused) return hipErrorInvalidValue;
  counted_launch(kCloseKernels[v], dim3(1), dim3(block), 0, s, args);
  return hipGetLastError();
}

// 512 threads as iterate_kernel<512>, whatever the context's loop uses: the persistent launches' summation order.
hipError_t launch_evaluate(hipStream_t s, const EvalArgs& args, uint32_t rows_per_pose, uint32_t poses) {
  if (rows_per_pose < 1 || rows_per_pose > (uint32_t)kMaxIterBlocks || poses < 1 ||
      (uint64_t)rows_per_pose * poses > (uint64_t)kEvalRowBudget || args.poses == nullptr || args.rows == nullptr)
    return hipErrorInvalidValue;
  counted_launch(evaluate_kernel<512>, dim3(rows_per_pose, poses), dim3(512), 0, s, args);
  return hipGetLastError();
}

hipError_t launch_evaluate_fold(hipStream_t s, const double* rows, uint32_t rows_per_pose, uint32_t poses, double* out) {
  if (rows_per_pose < 1 || poses < 1 || (uint64_t)rows_per_pose * poses > (uint64_t)kEvalRowBudget) return hipErrorInvalidValue;
  counted_launch(evaluate_fold_kernel, dim3(poses), dim3(512), 0, s, rows, rows_per_pose, out);
  return hipGetLastError();
}

hipError_t launch_point_terms(hipStream_t s, const PointArgs& args) {
  if (args.scan == nullptr || args.table == nullptr || args.counters == nullptr || (args.keys == nullptr) != (args.idx == nullptr))
    return hipErrorInvalidValue;
  if (args.n == 0) return hipSuccess;
  counted_launch(point_terms_kernel, dim3((args.n + 255u) / 256u), dim3(256), 0, s, args);
  return hipGetLastError();
}

hipError_t launch_gate_decide(hipStream_t s, const GateArgs& args) {
  if (args.n == 0) return hipSuccess;
  counted_launch(gate_decide_kernel, dim3((args.n + 255u) / 256u), dim3(256), 0, s, args);
  return hipGetLastError();
}

hipError_t launch_point_pick(hipStream_t s, const PointPickArgs& args) {
  if (args.counters == nullptr || args.out == nullptr || args.n_quantiles > (uint32_t)kPointQuantiles ||
      (args.n_quantiles > 0 && args.n > 0 && args.sorted == nullptr))
    return hipErrorInvalidValue;
  counted_launch(point_pick_kernel, dim3(1), dim3(64), 0, s, args);
  return hipGetLastError();
}

hipError_t launch_solve_step(hipStream_t s, const double* packed27, double cosine_threshold,
                             double translation_sq_threshold, int force_pivoted, double* out20) {
  counted_launch(solve_step_kernel, dim3(1), dim3(64), 0, s, packed27, cosine_threshold, translation_sq_threshold, force_pivoted,
                 out20);
  return hipGetLastError();
}

hipError_t launch_fold_rows(hipStream_t s, const double* rows, uint32_t nrows, const AlignState* state,
                            double* sums) {
  counted_launch(fold_rows_kernel, dim3(1), dim3(1024), 0, s, rows, nrows, state, sums);
  return hipGetLastError();
}

hipError_t launch_gather_scan(hipStream_t s, const uint32_t* perm, uint32_t m, const double* pts, const double* covs,
                              const unsigned long long* idx, double* out_pts, double* out_covs, unsigned long long* out_idx) {
  if (m == 0) return hipSuccess;
  counted_launch(gather_scan_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, s, perm, m, pts, covs, idx, out_pts, out_covs,
                 out_idx);
  return hipGetLastError();
}

hipError_t launch_pack_scan(hipStream_t s, const double* points_aos, const double* covs_aos,
                            uint32_t n, double* soa, uint64_t stride, uint32_t* asym, uint32_t seq) {
  if (n == 0) return hipSuccess;
  counted_launch(pack_scan_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, points_aos, covs_aos, n, soa, stride, asym, seq);
  return hipGetLastError();
}

uint32_t pack_arena_unit() { return 8u * kPackArenaBlock; }   // 2 048 points = 196 KB per unit
hipError_t launch_pack_arena(hipStream_t s, const void* arena_points, const void* arena_covs, uint32_t n,
                             const uint32_t* flags, bool wait, uint32_t seq, uint32_t spin_limit, double* aos_pts, double* aos_cov,
                             double* soa, uint64_t stride, uint32_t* asym) {
  if (n == 0) return hipSuccess;
  // few enough workgroups that the ones still waiting for their unit are a trickle of PCIe reads, enough of them that
  // 3 MB of loads are in flight; small LDS and 256 threads so that they find room beside other contexts' launches
  const uint32_t grid = std::min<uint32_t>(blocks_for(n, kPackArenaBlock), 128u);
  counted_launch(pack_arena_kernel, dim3(grid), dim3(kPackArenaBlock), 0, s, static_cast<const char*>(arena_points),
                 static_cast<const char*>(arena_covs), n, pack_arena_unit(), flags, wait ? 1u : 0u, seq, spin_limit, aos_pts,
                 aos_cov, soa, stride, asym);
  return hipGetLastError();
}

}  // namespace vgicp
