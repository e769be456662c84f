// ndt_sweep.hpp -- the derivative sweep (computeDerivatives + updateDerivatives + neighbour lookup,
// include/ndt_omp/ndt_omp_impl2.hpp:196-305, 503-532, 566-619; voxel_grid_covariance_omp_impl.hpp:373-442).
#pragma once
#include "ndt_types.hpp"
#include "ndt_math.hpp"
#include "ndt_newton.hpp"
#include <type_traits>

// ------------------------------------------------------------------------------------ derivative sweep
// One (point, voxel) evaluation: updateDerivatives (ndt_omp_impl2.hpp:566-619) with the Jacobian /
// Hessian patterns of computePointDerivatives_AngleAxisd (impl2:503-532) folded in (J and Hp are never
// materialised).  f32 ops single, left to right; f64 accumulation.  `w` = weight multiplier of the hit
// (ndt_pca compounding, applied as a suffix product; unused for ndt_omp).
struct NoHook { __device__ __forceinline__ void operator()() const {} };

// `mid` runs between the gradient part and the 36 Hessian terms, where the fewest temporaries are live: the sweep uses it
// to issue the NEXT batch's record loads so that their L2 latency overlaps the Hessian arithmetic.
// SAN (KDTREE modes only): radiusSearch also returns leaves whose inverse covariance is non-finite (no nr_points re-check,
// voxel_grid_covariance_omp.h:505-534); the reference rejects such a hit before touching the sums (impl2:588-589), so the
// operands of a rejected hit are zeroed first -- "e = 0" alone would still add 0 * NaN.
// ORD: evaluation order of the three-term f32 sums of impl2:581, 594-613 (4-wide Eigen inner products whose fourth term is a structural
// zero).  The reference leaves it to Eigen 3.3 and the SSE level it is compiled for (CMakeLists.txt:6,11: -msse4.2), and neither can
// be observed here.  0 = (t0 + t1) + t2: Eigen's scalar redux, the canonical choice of the committed parity fixtures;
// 1 = (t0 + t2) + t1: the lane pairing of Eigen 3.3's SSE predux<Packet4f>, (a0 + a2) + (a1 + a3) with a3 = 0.  Same instruction count
// either way; selected per engine with mi355ndt_set_option(MI355NDT_OPT_F32_SUM_ORDER) so that a maintainer who pins the reference on
// a real build (tools/pin_reference) can switch to the order that build shows.
template <int ORD>
__device__ __forceinline__ float sum3(float t0, float t1, float t2) { return ORD == 1 ? (t0 + t2) + t1 : (t0 + t1) + t2; }

// The part of an evaluation that the score needs (impl2:574-589): y = C u, q = u . y, the exponential, e1 and the validity gate.  Returns the
// gate; `s_inc` is the hit's (gated) score term.  eval_hit goes on from here, eval_score adds s_inc and is done.
template <int ORD>
__device__ __forceinline__ bool eval_prefix(const float u[3], const float C[9], const double d1, const float d2f, const bool ok_in,
                                            const double* __restrict__ exp_tab, float y[3], float& e1, float& s_inc) {
#pragma unroll
  for (int j = 0; j < 3; j++) y[j] = sum3<ORD>(u[0] * C[j], u[1] * C[3 + j], u[2] * C[6 + j]);
  const float qf = sum3<ORD>(u[0] * y[0], u[1] * y[1], u[2] * y[2]);
  const float e0 = ndtm::exp_f32arg((-d2f * qf) * 0.5f, exp_tab);                // impl2:581: exp in f64 on the f32 argument, rounded to f32
  s_inc = (float)(-d1 * (double)e0);                                             // impl2:583
  e1 = d2f * e0;                                                                 // impl2:585
  // impl2:588-589, branch-free: a rejected hit (or an idle lane, ok_in = false) multiplies every term by e = 0 and so
  // adds +0 to all 43 sums (all operands are finite here: dead voxels never enter the queue).
  const bool ok = ok_in && !(e1 > 1.f || e1 < 0.f || e1 != e1);
  s_inc = ok ? s_inc : 0.f;
  return ok;
}

template <bool PCA, typename Mid = NoHook, bool SAN = false, int ORD = 0>
__device__ __forceinline__ void eval_hit(const float u_in[3], const float r[3], const float C_in[9],
                                         const double d1, const float d2f, const double w, const bool ok_in, double acc[43],
                                         const double* __restrict__ exp_tab, Mid mid = Mid()) {
  float u[3] = {u_in[0], u_in[1], u_in[2]}, C[9];
#pragma unroll
  for (int a = 0; a < 9; a++) C[a] = C_in[a];
  float y[3], e1, s_inc;
  const bool ok = eval_prefix<ORD>(u, C, d1, d2f, ok_in, exp_tab, y, e1, s_inc);
  float e = (float)((double)e1 * d1);                                            // impl2:592
  e = ok ? e : 0.f;
  if (SAN) {
#pragma unroll
    for (int a = 0; a < 3; a++) { u[a] = ok ? u[a] : 0.f; y[a] = ok ? y[a] : 0.f; }
#pragma unroll
    for (int a = 0; a < 9; a++) C[a] = ok ? C[a] : 0.f;
  }
  // CJ = c_inv4 * point_gradient4 (impl2:594): columns 0..2 are C itself
  float CJ[3][6];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    CJ[a][0] = C[a * 3 + 0]; CJ[a][1] = C[a * 3 + 1]; CJ[a][2] = C[a * 3 + 2];
    CJ[a][3] = C[a * 3 + 1] * (-r[2]) + C[a * 3 + 2] * r[1];
    CJ[a][4] = C[a * 3 + 0] * r[2] + C[a * 3 + 2] * (-r[0]);
    CJ[a][5] = C[a * 3 + 0] * (-r[1]) + C[a * 3 + 1] * r[0];
  }
  float v[6];
#pragma unroll
  for (int k = 0; k < 6; k++) v[k] = sum3<ORD>(u[0] * CJ[0][k], u[1] * CJ[1][k], u[2] * CJ[2][k]);   // impl2:595
  // w * term: the product is a single rounding away from the reference's nested multiplies (both ~1e-16)
#define NDT_ACC(slot, val) do { if (PCA) acc[slot] = fma(w, (double)(val), acc[slot]); else acc[slot] += (double)(val); } while (0)
  NDT_ACC(0, s_inc);
#pragma unroll
  for (int k = 0; k < 6; k++) NDT_ACC(1 + k, e * v[k]);                                        // impl2:597
  // z_i[j] = y * Hp_block_i (impl2:607) -- nine non-zero entries (impl2:522-530)
  float Z[3][3];
  Z[0][0] = y[1] * (-r[1]) + y[2] * (-r[2]);
  Z[1][0] = y[0] * r[1];
  Z[2][0] = y[0] * r[2];
  Z[0][1] = y[1] * r[0];
  Z[1][1] = y[0] * (-r[0]) + y[2] * (-r[2]);
  Z[2][1] = y[1] * r[2];
  Z[0][2] = y[2] * r[0];
  Z[1][2] = y[2] * r[1];
  Z[2][2] = y[0] * (-r[0]) + y[1] * (-r[1]);
  __builtin_amdgcn_sched_barrier(0);
  mid();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      // JCJ[j][i] = (J^T CJ)(j,i) (impl2:601)
      float jcj;
      if (j < 3) jcj = CJ[j][i];
      else if (j == 3) jcj = (-r[2]) * CJ[1][i] + r[1] * CJ[2][i];
      else if (j == 4) jcj = r[2] * CJ[0][i] + (-r[0]) * CJ[2][i];
      else jcj = (-r[1]) * CJ[0][i] + r[0] * CJ[1][i];
      // z_i[j] is a structural zero outside the rotation block; "+ (+-0)" never changes a value that reaches the f64 sums
      // (it can only turn a -0 term into +0, and adding either to an accumulator is a no-op), so the add is skipped there
      float t = ((-d2f) * v[i]) * v[j];
      if (i >= 3 && j >= 3) t = t + Z[i - 3][j - 3];
      const float h = e * (t + jcj);                                                           // impl2:611-613
      NDT_ACC(7 + i * 6 + j, h);
    }
  }
#undef NDT_ACC
}

// ------------------------------------------------------------------------------------ the Euler-angle pose model (PM = 1)
// MI355NDT_OPT_POSE_MODEL = 1: the evaluation of include/ndt_omp/ndt_omp_impl.hpp.  updateDerivatives (impl.hpp:483-535) is impl2's, operation
// for operation -- the same eval_prefix, the same sum3<ORD>, one rounding per f32 operation, the same 43 f64 sums -- but the point Jacobian and the
// point Hessian are those of the f32 computePointDerivatives (impl.hpp:397-438): eight entries x . j_ang row and the six vectors a .. f = x . h_ang
// rows, taken from the ORIGINAL point x (staged where eval_hit finds R x) and the pair's 23 rows `rw` (ndtm::euler_rows: wave-uniform, so they
// arrive through scalar loads).  Structural zeros of the 4 x 6 / 24 x 6 patterns are skipped as in eval_hit: Jacobian entry (0, 3), the first
// components of a, b, c, the fourth lane of every inner product.  ndt_omp only (ndt_pca_impl.hpp has the weight commented out), exact arithmetic only.
// The rows are written by the launch before the sweep and by nobody during it: read through the constant address space, a wave-uniform
// address makes every one of them a scalar load.
typedef const __attribute__((address_space(4))) float* EulerRows;
__device__ __forceinline__ EulerRows euler_rows_of_pair(const float* rows, const int b) {
  return (EulerRows)(unsigned long long)(rows + (size_t)__builtin_amdgcn_readfirstlane(b) * EULER_ROW_WORDS);
}
template <typename Mid = NoHook, bool SAN = false, int ORD = 0>
__device__ __forceinline__ void eval_hit_euler(const float u_in[3], const float x[3], const float C_in[9], const EulerRows rw,
                                               const double d1, const float d2f, const bool ok_in, double acc[43],
                                               const double* __restrict__ exp_tab, Mid mid = Mid()) {
  float u[3] = {u_in[0], u_in[1], u_in[2]}, C[9];
#pragma unroll
  for (int a = 0; a < 9; a++) C[a] = C_in[a];
  float y[3], e1, s_inc;
  const bool ok = eval_prefix<ORD>(u, C, d1, d2f, ok_in, exp_tab, y, e1, s_inc);
  float e = (float)((double)e1 * d1);                                            // impl.hpp:508
  e = ok ? e : 0.f;
  if (SAN) {
#pragma unroll
    for (int a = 0; a < 3; a++) { u[a] = ok ? u[a] : 0.f; y[a] = ok ? y[a] : 0.f; }
#pragma unroll
    for (int a = 0; a < 9; a++) C[a] = ok ? C[a] : 0.f;
  }
  // x_j_ang = j_ang * x4 (impl.hpp:403): the Jacobian's columns 3..5 are (0, xj0, xj1), (xj2, xj3, xj4), (xj5, xj6, xj7) (impl.hpp:405-412)
  float xj[8];
#pragma unroll
  for (int k = 0; k < 8; k++) xj[k] = sum3<ORD>(rw[3 * k] * x[0], rw[3 * k + 1] * x[1], rw[3 * k + 2] * x[2]);
  // CJ = c_inv4 * point_gradient4 (impl.hpp:510): columns 0..2 are C itself
  float CJ[3][6];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    CJ[a][0] = C[a * 3 + 0]; CJ[a][1] = C[a * 3 + 1]; CJ[a][2] = C[a * 3 + 2];
    CJ[a][3] = C[a * 3 + 1] * xj[0] + C[a * 3 + 2] * xj[1];
    CJ[a][4] = sum3<ORD>(C[a * 3 + 0] * xj[2], C[a * 3 + 1] * xj[3], C[a * 3 + 2] * xj[4]);
    CJ[a][5] = sum3<ORD>(C[a * 3 + 0] * xj[5], C[a * 3 + 1] * xj[6], C[a * 3 + 2] * xj[7]);
  }
  float v[6];
#pragma unroll
  for (int k = 0; k < 6; k++) v[k] = sum3<ORD>(u[0] * CJ[0][k], u[1] * CJ[1][k], u[2] * CJ[2][k]);   // impl.hpp:511
  acc[0] += (double)s_inc;
#pragma unroll
  for (int k = 0; k < 6; k++) acc[1 + k] += (double)(e * v[k]);                                  // impl.hpp:513
  // x_h_ang = h_ang * x4 (impl.hpp:416) and z = (x_trans4 * c_inv4) * point_hessian block (impl.hpp:523): the blocks are a b c / b d e / c e f
  // (impl.hpp:428-436), so six inner products serve the nine entries
  float xh[15];
#pragma unroll
  for (int k = 0; k < 15; k++) xh[k] = sum3<ORD>(rw[24 + 3 * k] * x[0], rw[24 + 3 * k + 1] * x[1], rw[24 + 3 * k + 2] * x[2]);
  const float za = y[1] * xh[0] + y[2] * xh[1];
  const float zb = y[1] * xh[2] + y[2] * xh[3];
  const float zc = y[1] * xh[4] + y[2] * xh[5];
  const float zd = sum3<ORD>(y[0] * xh[6], y[1] * xh[7], y[2] * xh[8]);
  const float ze = sum3<ORD>(y[0] * xh[9], y[1] * xh[10], y[2] * xh[11]);
  const float zf = sum3<ORD>(y[0] * xh[12], y[1] * xh[13], y[2] * xh[14]);
  const float Z[3][3] = {{za, zb, zc}, {zb, zd, ze}, {zc, ze, zf}};
  __builtin_amdgcn_sched_barrier(0);
  mid();
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      // JCJ[j][i] = (J^T CJ)(j,i) (impl.hpp:517)
      float jcj;
      if (j < 3) jcj = CJ[j][i];
      else if (j == 3) jcj = xj[0] * CJ[1][i] + xj[1] * CJ[2][i];
      else if (j == 4) jcj = sum3<ORD>(xj[2] * CJ[0][i], xj[3] * CJ[1][i], xj[4] * CJ[2][i]);
      else jcj = sum3<ORD>(xj[5] * CJ[0][i], xj[6] * CJ[1][i], xj[7] * CJ[2][i]);
      float t = ((-d2f) * v[i]) * v[j];
      if (i >= 3 && j >= 3) t = t + Z[i - 3][j - 3];
      const float h = e * (t + jcj);                                                           // impl.hpp:527-529
      acc[7 + i * 6 + j] += (double)h;
    }
  }
}

// ------------------------------------------------------------------------------------ pcl::NormalDistributionsTransform (PM = 2)
// MI355NDT_OPT_NDT_CLASS = 1: PCL's own class, which is impl.hpp with the f32 substitutions undone -- updateDerivatives in f64 from end to end
// (the structure of impl.hpp:482-535, the terms updateHessian writes in f64 at impl.hpp:598-640) over the f64 computePointDerivatives
// (impl.hpp:442-479).  u = the f32 moved point widened minus the leaf's f64 mean, C = the leaf's f64 inverse covariance (row-major; not assumed
// symmetric), x = the ORIGINAL point widened, `rw` = the pair's 23 rows as doubles.
//   e = d1 d2 exp(-d2 u'C u / 2), rejected as impl.hpp:504 rejects;  g_i += e u.(C J_i);
//   H_ij += e (-d2 (u.C J_i)(u.C J_j) + u.(C Hp_ij) + J_j.(C J_i)), all 36 of them: nothing is mirrored, so the 43 sums keep the row layout and tree.
// u.(C w) is evaluated as (u'C).w for every w (one row vector per hit instead of a matrix-vector product per term): the same number up to the
// rounding of an f64 inner product, which is what the class is held to (1e-11 of the largest entry against tools/ndt_pcl_ref.py).  Inner products
// are fused (fma): this body restates no f32 recipe whose roundings would have to be kept apart.
// The eight Jacobian and fifteen Hessian-block entries depend on the point alone.  They are computed here, per hit, from x and the rows (69 scalar
// loads + 69 f64 operations, about a fifth of a hit's arithmetic) and not once per point in phase A: staged, they would be 184 bytes a point,
// 94 KB of LDS per workgroup at the two super-tile buffers of the K = 27 item -- more than two workgroups per CU can have.
// The rows are wave-uniform and read through the constant address space: scalar loads on demand, no LDS, no vector register until an operation
// needs the value as an operand.
typedef const __attribute__((address_space(4))) double* PclRows;
struct PclCtx { PclRows rows; const double* icov64; };     // the pair's rows; the f64 inverse covariances of the pair's target grid
__device__ __forceinline__ PclRows pcl_rows_of_pair(const double* rows, const int b) {
  return (PclRows)(unsigned long long)(rows + (size_t)__builtin_amdgcn_readfirstlane(b) * EULER_ROW_WORDS);
}
__device__ __forceinline__ double dot3(const double a0, const double b0, const double a1, const double b1, const double a2, const double b2) {
  return fma(a2, b2, fma(a1, b1, a0 * b0));
}
template <typename Mid = NoHook>
__device__ __forceinline__ void eval_hit_pcl(const double u_in[3], const float xf[3], const double C_in[9], const PclRows rw,
                                             const double d1, const double d2, const bool ok_in, double acc[43], Mid mid = Mid()) {
  double u[3] = {u_in[0], u_in[1], u_in[2]}, C[9];
#pragma unroll
  for (int a = 0; a < 9; a++) C[a] = C_in[a];
  double uC[3];                                                                  // u' C
#pragma unroll
  for (int k = 0; k < 3; k++) uC[k] = dot3(u[0], C[k], u[1], C[3 + k], u[2], C[6 + k]);
  const double e0 = exp(-d2 * dot3(uC[0], u[0], uC[1], u[1], uC[2], u[2]) / 2);
  const double e1 = d2 * e0;
  // (radiusSearch returns leaves without a usable inverse covariance as well: a rejected hit adds +0 to every sum, so its operands go first)
  const bool ok = ok_in && !(e1 > 1.0 || e1 < 0.0 || e1 != e1);
  const double e = ok ? e1 * d1 : 0.0;
  acc[0] += ok ? -d1 * e0 : 0.0;
#pragma unroll
  for (int a = 0; a < 3; a++) { u[a] = ok ? u[a] : 0.0; uC[a] = ok ? uC[a] : 0.0; }
#pragma unroll
  for (int a = 0; a < 9; a++) C[a] = ok ? C[a] : 0.0;
  const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
  // point_gradient_ columns 3..5: (0, xj0, xj1), (xj2, xj3, xj4), (xj5, xj6, xj7) (impl.hpp:446-453)
  double xj[8];
#pragma unroll
  for (int k = 0; k < 8; k++) xj[k] = dot3(x[0], rw[3 * k], x[1], rw[3 * k + 1], x[2], rw[3 * k + 2]);
  const double Jr[3][3] = {{0.0, xj[2], xj[5]}, {xj[0], xj[3], xj[6]}, {xj[1], xj[4], xj[7]}};   // rows of J's rotation columns
  double v[6] = {uC[0], uC[1], uC[2], fma(uC[2], Jr[2][0], uC[1] * Jr[1][0]), dot3(uC[0], Jr[0][1], uC[1], Jr[1][1], uC[2], Jr[2][1]),
                 dot3(uC[0], Jr[0][2], uC[1], Jr[1][2], uC[2], Jr[2][2])};
#pragma unroll
  for (int k = 0; k < 6; k++) acc[1 + k] = fma(e, v[k], acc[1 + k]);
  // u.(C Hp_ij): the blocks are a b c / b d e / c e f (impl.hpp:460-477), a, b, c without a first component
  double Z[3][3];
  {
    double xh[15];
#pragma unroll
    for (int k = 0; k < 15; k++) xh[k] = dot3(x[0], rw[24 + 3 * k], x[1], rw[24 + 3 * k + 1], x[2], rw[24 + 3 * k + 2]);
    const double za = fma(uC[2], xh[1], uC[1] * xh[0]), zb = fma(uC[2], xh[3], uC[1] * xh[2]), zc = fma(uC[2], xh[5], uC[1] * xh[4]);
    const double zd = dot3(uC[0], xh[6], uC[1], xh[7], uC[2], xh[8]), ze = dot3(uC[0], xh[9], uC[1], xh[10], uC[2], xh[11]);
    const double zf = dot3(uC[0], xh[12], uC[1], xh[13], uC[2], xh[14]);
    Z[0][0] = za; Z[0][1] = zb; Z[0][2] = zc; Z[1][0] = zb; Z[1][1] = zd; Z[1][2] = ze; Z[2][0] = zc; Z[2][1] = ze; Z[2][2] = zf;
  }
  __builtin_amdgcn_sched_barrier(0);
  mid();
  __builtin_amdgcn_sched_barrier(0);
  // one row of H at a time: C J_i is three doubles that live for six terms (C J as a whole would be eighteen, for all thirty-six); the
  // scheduling barrier between the rows keeps the compiler from interleaving them back into that
#pragma unroll
  for (int i = 0; i < 6; i++) {
    // C J_i: a column of C for a translation (J_i a unit vector); only the three rotation columns cost a product
    double CJi[3];
#pragma unroll
    for (int a = 0; a < 3; a++)
      CJi[a] = i < 3 ? C[a * 3 + i] : (i == 3 ? fma(C[a * 3 + 2], Jr[2][0], C[a * 3 + 1] * Jr[1][0])
                                              : dot3(C[a * 3 + 0], Jr[0][i < 3 ? 0 : i - 3], C[a * 3 + 1], Jr[1][i < 3 ? 0 : i - 3], C[a * 3 + 2], Jr[2][i < 3 ? 0 : i - 3]));
    const double dvi = -d2 * v[i];
#pragma unroll
    for (int j = 0; j < 6; j++) {
      // J_j . (C J_i)
      const int c = j < 3 ? 0 : j - 3;
      double t = j < 3 ? CJi[j] : (j == 3 ? fma(Jr[2][0], CJi[2], Jr[1][0] * CJi[1]) : dot3(Jr[0][c], CJi[0], Jr[1][c], CJi[1], Jr[2][c], CJi[2]));
      if (i >= 3 && j >= 3) t += Z[i - 3][j - 3];
      acc[7 + i * 6 + j] = fma(e, fma(dvi, v[j], t), acc[7 + i * 6 + j]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Score-only evaluation (MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP): eval_hit's prefix and the same term added to the same accumulator, for the
// last sweep of an align, whose gradient and Hessian are never read.
template <bool PCA, int ORD = 0>
__device__ __forceinline__ void eval_score(const float u[3], const float C[9], const double d1, const float d2f, const double w, const bool ok_in,
                                           double& acc0, const double* __restrict__ exp_tab) {
  float y[3], e1, s_inc;
  eval_prefix<ORD>(u, C, d1, d2f, ok_in, exp_tab, y, e1, s_inc);
  if (PCA) acc0 = fma(w, (double)s_inc, acc0); else acc0 += (double)s_inc;
}

// ------------------------------------------------------------------------------------ tolerance arithmetic (ORD = 2)
// MI355NDT_OPT_ARITH = 1: the same evaluation -- updateDerivatives with the patterns of computePointDerivatives_AngleAxisd folded in -- priced
// for north_star's tolerance (trans < 1e-4 m, rot < 1e-5 rad) instead of one separately rounded operation per step of the reference recipe.  What changes against eval_hit:
//   * fused multiply-adds, one v_exp_f32 (exp(-d2 q / 2) = 2^(kq q)) instead of the f64 table + polynomial, d1 as f32;
//   * the inverse covariance as a symmetric matrix (six entries), so J^T C J is symmetric and H = S + [0 0; 0 Z] with S symmetric:
//     21 sums for S, and the asymmetric part (impl2:522-530, 607) Z = r y^T - (y . r) I needs only A = sum e r y^T (9 sums; the trace term
//     is recovered from A's diagonal when the row is written);
//   * 37 f32 accumulators per lane instead of 43 f64 ones; a lane adds ~35 terms into them per work item (512 points) before they are widened
//     and go through the f64 wave tree and the f64 row sums of the update as before.
// What does NOT change: the point transform and the cell lookup (uncontracted f32, SURVEY.md H3: which leaf a point meets is discontinuous),
// the validity gate of impl2:588-589, the Newton update.  This mode is held to the tolerance, not to bits
// (tests/test_tolerance_mode.py, bench.py `tolerance_mode`).
#define NACC_F 37
__host__ __device__ constexpr int fsym(int i, int j) { return i <= j ? 7 + i * 6 - i * (i - 1) / 2 + (j - i) : 7 + j * 6 - j * (j - 1) / 2 + (i - j); }
#define FA_BASE 28             // A[i][j] = a[FA_BASE + 3 i + j]
// ... its prefix (as eval_prefix): y, q, one v_exp_f32, e1, the gate; `s` is the hit's weighted, gated score term
template <bool PCA>
__device__ __forceinline__ bool eval_prefix_fast(const float u[3], const float c[6], const float d1f, const float d2f, const float kq, const float w,
                                                 const bool ok_in, float y[3], float& e1, float& s) {
  const float c00 = c[0], c01 = c[1], c02 = c[2], c11 = c[3], c12 = c[4], c22 = c[5];
  y[0] = fmaf(c02, u[2], fmaf(c01, u[1], c00 * u[0]));
  y[1] = fmaf(c12, u[2], fmaf(c11, u[1], c01 * u[0]));
  y[2] = fmaf(c22, u[2], fmaf(c12, u[1], c02 * u[0]));
  const float q = fmaf(u[2], y[2], fmaf(u[1], y[1], u[0] * y[0]));
  const float e0 = __builtin_amdgcn_exp2f(kq * q);                               // impl2:581
  e1 = d2f * e0;                                                                 // impl2:585
  const bool ok = ok_in && !(e1 > 1.f || e1 < 0.f || e1 != e1);                  // impl2:588-589
  s = -d1f * e0;                                                                 // impl2:583
  if (PCA) s *= w;
  s = ok ? s : 0.f;
  return ok;
}
template <bool PCA, typename Mid = NoHook>
__device__ __forceinline__ void eval_hit_fast(const float u[3], const float r[3], const float c[6], const float d1f, const float d2f, const float kq,
                                              const float w, const bool ok_in, float a[NACC_F], Mid mid = Mid()) {
  const float c00 = c[0], c01 = c[1], c02 = c[2], c11 = c[3], c12 = c[4], c22 = c[5];
  float y[3], e1, s;
  const bool ok = eval_prefix_fast<PCA>(u, c, d1f, d2f, kq, w, ok_in, y, e1, s);
  float e = e1 * d1f;                                                            // impl2:592
  if (PCA) e *= w;
  e = ok ? e : 0.f;
  a[0] += s;
  // v = J^T y = [y ; r x y] (impl2:595 with CJ's columns 0..2 = C)
  float v[6] = {y[0], y[1], y[2], fmaf(r[1], y[2], -(r[2] * y[1])), fmaf(r[2], y[0], -(r[0] * y[2])), fmaf(r[0], y[1], -(r[1] * y[0]))};
#pragma unroll
  for (int k = 0; k < 6; k++) a[1 + k] = fmaf(e, v[k], a[1 + k]);                // impl2:597
  __builtin_amdgcn_sched_barrier(0);
  mid();
  __builtin_amdgcn_sched_barrier(0);
  // M = C (-[r]x): columns 3..5 of CJ (impl2:594)
  const float C[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
  float M[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    M[i][0] = fmaf(C[i][2], r[1], -(C[i][1] * r[2]));
    M[i][1] = fmaf(C[i][0], r[2], -(C[i][2] * r[0]));
    M[i][2] = fmaf(C[i][1], r[0], -(C[i][0] * r[1]));
  }
  float dv[6];
#pragma unroll
  for (int k = 0; k < 6; k++) dv[k] = -d2f * v[k];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = i; j < 3; j++) a[fsym(i, j)] = fmaf(e, fmaf(dv[i], v[j], C[i][j]), a[fsym(i, j)]);          // translation block
#pragma unroll
    for (int k = 0; k < 3; k++) a[fsym(i, 3 + k)] = fmaf(e, fmaf(dv[i], v[3 + k], M[i][k]), a[fsym(i, 3 + k)]);   // translation x rotation
  }
  // rotation block of J^T C J: [r]x M (symmetric: six entries)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float rr0 = fmaf(r[1], M[2][k], -(r[2] * M[1][k]));
    const float rr1 = fmaf(r[2], M[0][k], -(r[0] * M[2][k]));
    const float rr2 = fmaf(r[0], M[1][k], -(r[1] * M[0][k]));
    if (k >= 0) a[fsym(3, 3 + k)] = fmaf(e, fmaf(dv[3], v[3 + k], rr0), a[fsym(3, 3 + k)]);
    if (k >= 1) a[fsym(4, 3 + k)] = fmaf(e, fmaf(dv[4], v[3 + k], rr1), a[fsym(4, 3 + k)]);
    if (k >= 2) a[fsym(5, 3 + k)] = fmaf(e, fmaf(dv[5], v[3 + k], rr2), a[fsym(5, 3 + k)]);
  }
  // A = e r y^T: the point-Hessian term (impl2:522-530, 607), z_{3+i}[3+j] = r_i y_j - delta_ij (y . r)
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float er = e * r[i];
#pragma unroll
    for (int j = 0; j < 3; j++) a[FA_BASE + 3 * i + j] = fmaf(er, y[j], a[FA_BASE + 3 * i + j]);
  }
}
// ... and its score-only form (as eval_score for eval_hit): the prefix, the same f32 sum a[0]
template <bool PCA>
__device__ __forceinline__ void eval_score_fast(const float u[3], const float c[6], const float d1f, const float d2f, const float kq,
                                                const float w, const bool ok_in, float& a0) {
  float y[3], e1, s;
  eval_prefix_fast<PCA>(u, c, d1f, d2f, kq, w, ok_in, y, e1, s);
  a0 += s;
}
// A score-only work item's row: the lane sums of the score added with the pairwise tree of the reduce-scatter below (lanes l / l^32, then
// l^16, ... l^1: the same operand pairs, so the same bits), then the score and the hit count are the only words of the row written.
__device__ __forceinline__ double score_tree(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the 37 sums of a lane -> the 43 entries of a partial row (score, g, H row-major), widened
__device__ __forceinline__ void fast_acc_to_row(const float a[NACC_F], double acc[43]) {
#pragma unroll
  for (int k = 0; k < 7; k++) acc[k] = (double)a[k];
  const double tr = ((double)a[FA_BASE] + (double)a[FA_BASE + 4]) + (double)a[FA_BASE + 8];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      double h = (double)a[fsym(i, j)];
      if (i >= 3 && j >= 3) { h += (double)a[FA_BASE + 3 * (i - 3) + (j - 3)]; if (i == j) h -= tr; }
      acc[7 + i * 6 + j] = h;
    }
  }
}

// Neighbour offset `a` (0..2) of probe q for a K-probe search, resolved at compile time in the sweep
// (same tables and order as c_off above).
__host__ __device__ constexpr int probe_off(int K, int q, int a) {
  const int o7[7][3] = {{0,0,0},{1,0,0},{-1,0,0},{0,1,0},{0,-1,0},{0,0,1},{0,0,-1}};
  const int o26[26][3] = {{-1,-1,-1}, {-1,0,-1}, {-1,1,-1}, {0,-1,-1}, {0,0,-1}, {0,1,-1}, {1,-1,-1}, {1,0,-1}, {1,1,-1}, {-1,-1,0}, {0,-1,0}, {1,-1,0}, {-1,0,0}, {1,1,1}, {1,0,1}, {1,-1,1}, {0,1,1}, {0,0,1}, {0,-1,1}, {-1,1,1}, {-1,0,1}, {-1,-1,1}, {1,1,0}, {0,1,0}, {-1,1,0}, {1,0,0}};
  // K == 27: the KDTREE emulation -- every cell of the 3x3x3 block around the point (centre included)
  return K == 1 ? 0 : (K == 7 ? o7[q][a] : (K == 26 ? o26[q][a] : (a == 0 ? q % 3 - 1 : (a == 1 ? (q / 3) % 3 - 1 : q / 9 - 1))));
}

#define Q_GROUP 7                         // probes between queue drains
#define ID_BITS 23                        // queue entry = staging slot << 23 | voxel id
#define WAVES   (SWEEP_THREADS / 64)

// The sweep.  Work decomposition (MI355X-first):
//   work item = one wave-quarter (CHUNK_PTS/4 = 512 consecutive points) of one 2048-point chunk of one active pair, taken by
//     ONE persistent wave from a per-XCD queue; a workgroup is just four such independent waves.
//   phase A (probe, lane = point): transform the points of a super-tile (1, 2 or 4 tiles of 64) in f32, probe their K neighbour
//     cells in the rank-bitmap, and push every hit as a 4-byte entry into the wave's LDS queue (ballot + popcount compaction).
//   phase B (evaluate, lane = hit): lanes pull 64 queue entries at a time -- every lane busy no matter how the
//     hits were distributed over points -- read the staged point (LDS) and the 64-B voxel record, and add the
//     43 f64 terms into per-lane accumulators; the next batch's records are fetched in the middle of the current evaluation.
//   item end: flush the queue tail, fixed-tree wave reduction -> one 44-double partial row per (chunk, quarter).
// The partial rows depend only on (CHUNK_PTS, input order), never on the launch geometry or on which wave ran the item, so
// single and batched runs of one pair are bit-identical.
// -DNDT_TIMELINE: per-phase shader-clock stamps of every work item, summed over all waves into g_tl (read back through
// mi355ndt_debug_timeline; tools/sweep_timeline.py).  Costs ~10 % and is never part of the shipped library.
#ifdef NDT_TIMELINE
__device__ unsigned long long g_tl[16];
struct Timeline {                // one per wave: the counters and the last clock value
  unsigned long long t[16], last;
  __device__ __forceinline__ Timeline() { for (int k = 0; k < 16; k++) t[k] = 0; last = __builtin_readcyclecounter(); }
  __device__ __forceinline__ void stamp(const int k) {
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t_ = __builtin_readcyclecounter();
    t[k] += t_ - last; last = t_;
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void count(const int k = 7) { t[k] += 1; }          // (slot 7: work items)
  __device__ __forceinline__ void restart() { last = __builtin_readcyclecounter(); }
  __device__ __forceinline__ void flush(const int k0, const int k1) const { if ((threadIdx.x & 63) == 0) for (int k = k0; k < k1; k++) atomicAdd(&g_tl[k], t[k]); }
};
#else
struct Timeline {                // the shipped library: nothing
  __device__ __forceinline__ void stamp(int) {}
  __device__ __forceinline__ void count(int = 7) {}
  __device__ __forceinline__ void restart() {}
  __device__ __forceinline__ void flush(int, int) const {}
};
#endif
#define TL_STAMP(k) tl.stamp(k)
struct SweepCtl {               // 9 ints; two of them alternate: the sweep that reads one clears the other
  int n_active;                 // pairs whose next sweep is pending (entries of active_list)
  int next_item[8];             // per-XCD work-item cursors of the sweep
};
#define QUARTERS WAVES          // a chunk is reduced as 4 wave-quarters of CHUNK_PTS/4 points

// Per-instantiation tuning knobs (none of them changes a result bit).
#ifndef FAST_WPE7
#define FAST_WPE7 4            // tolerance arithmetic: 37 f32 accumulators instead of 43 f64 ones leave room for four waves per SIMD
#endif
#ifndef FAST_WPE1
#define FAST_WPE1 3            // ... DIRECT1: three (168 registers: no spill; measured 1,338 us per pca / 1 m launch against 1,554 with four)
#endif
#ifndef FAST_TP7
#define FAST_TP7 1
#endif
#ifndef FAST_TP1
#define FAST_TP1 2
#endif
#ifndef FAST_PIPE
#define FAST_PIPE 1
#endif
// LEAN (MI355NDT_OPT_SWEEP_WAVES; exact ndt_omp / DIRECT7 in the one-launch align alone): the same item body register-allocated for three
// waves per SIMD (168 VGPRs).  What it gives up for that: the mid-evaluation record prefetch, and the second tile of a probe group -- a
// super-tile is still two tiles (the staging geometry, the partial drains at its boundaries), probed one tile at a time.  Rows keep their bits:
// hits enter the queue in the same order, full batches leave it FIFO, the partial drains happen at the same boundaries with the same counts.
template <bool PCA, int K, int ORD = 0, bool LEAN = false>
struct SweepTune {
  static_assert(!LEAN || (!PCA && K == 7 && (ORD == 0 || ORD == 1)), "the lean body: exact ndt_omp / DIRECT7");
  static constexpr bool FAST = (ORD == 2);
  static constexpr int  WPE  = LEAN ? 3 : (FAST ? (K == 1 ? FAST_WPE1 : FAST_WPE7) : SWEEP_WPE);     // workgroups per CU = waves per SIMD
  static constexpr bool PIPE = LEAN ? false : (FAST ? (FAST_PIPE != 0) : true);                      // fetch batch k+1's records in the middle of batch k
  // tiles of a super-tile (8 = the whole work item); tolerance arithmetic: small super-tiles keep the LDS of a workgroup under a quarter of the CU's
  static constexpr int  TP   = FAST ? (K == 1 ? FAST_TP1 : FAST_TP7) : (K == 1 ? 8 : (K <= 7 ? 2 : 1));
  static constexpr int  TPP  = LEAN ? 1 : TP;                                                        // ... of which that many are probed together
};
static inline int sweep_wpe(int K, bool fast = false, bool lean = false) { return lean ? 3 : (fast ? (K == 1 ? FAST_WPE1 : FAST_WPE7) : SWEEP_WPE); }

// IT = tiles of 64 points per work item.  8 is the batch mode described above (a wave-quarter of a 2048-point chunk).
// FINE (latency mode): small items (IT = 1 or 2) dealt statically over ALL waves of the grid, for a sweep over one or a
// few pairs -- a single 65,536-point pair then offers 512-1024 items to the 2,048 resident waves instead of 128, and no wave
// claims anything with an atomic.  A pair's rows are then summed by k_update with the same rule over 4-row chunks of 4 * IT * 64
// points: its own fixed tree, not the batch mode's (results agree to the f64 rounding of the sums, ~1e-16 relative).
// `grid_of` (may be null): pair b is aligned against the target grid gd[grid_of[b]] instead of gd[b] (sequence mode: the frames'
// grids are built once, the keyframe policy picks which one a frame is matched against).
// One work item of the sweep: `IT` tiles of 64 consecutive points (item `rem`) of pair `b`, run by ONE wave -> one 44-double partial row.
// Shared by the lockstep kernel (k_sweep: one launch per Newton round) and the asynchronous one (k_align_async: one launch per align).
// ASYNC: the pair's pose is read, and its row is written, with agent-scope (sc1) accesses -- another workgroup wrote / will read them
// inside the same launch (ndt_async.hpp) -- and the FINE block reduction does not apply.
// ASYNC: the 21 pose words of pair state S (T: 12, Rj: 9) and its last_sweep flag (word 21), lane k holding word k -- one agent-scope
// (L1-bypassing) vector load, never the scalar cache: the pair's updater, some other workgroup of the same launch, rewrote them since the
// pair's previous sweep
#define POSE_W_LAST 21
__device__ __forceinline__ unsigned sweep_pose_words(const PairState* S) {
  static_assert(offsetof(PairState, T) == 0 && offsetof(PairState, Rj) == 48 && offsetof(PairState, last_sweep) == 4 * POSE_W_LAST, "pose words");
  const int lane = threadIdx.x & 63;
  unsigned w = 0;
  if (lane <= POSE_W_LAST) w = __hip_atomic_load((const gu32*)reinterpret_cast<const unsigned*>(S) + lane, RLX_AGENT);
  return w;
}

__device__ __forceinline__ void pose_from_words(const unsigned pose_w, float T[12], float Rj[9]) {
#pragma unroll
  for (int a = 0; a < 12; a++) T[a] = __uint_as_float(__builtin_amdgcn_readlane(pose_w, a));
#pragma unroll
  for (int a = 0; a < 9; a++) Rj[a] = __uint_as_float(__builtin_amdgcn_readlane(pose_w, 12 + a));
}

// A score-only work item's row: the lane sums of the score through score_tree, then the score and the hit count are the only words of
// the row written (agent scope: one-launch align only).
__device__ __forceinline__ void score_row_store(const double lane_score, double* P, const unsigned nhits, const int lane) {
  const double v = score_tree(lane_score);
  if (lane == 0) {
    gu64* PG = (gu64*)reinterpret_cast<unsigned long long*>(P);
    __hip_atomic_store(PG, (unsigned long long)__double_as_longlong(v), RLX_AGENT);
    __hip_atomic_store(PG + 43, (unsigned long long)__double_as_longlong((double)nhits), RLX_AGENT);
  }
}

// Fixed-order reduction of the wave's 43 lane sums -> one 44-double row at P.  Same pairwise tree as a 64-lane xor
// butterfly (distance 32, 16, 8, 4, 2, 1 -- so the same bits), but as a reduce-scatter: the distance-32 and -16
// levels use gfx950's v_permlane32_swap / v_permlane16_swap to exchange HALF of the values between lane halves /
// rows, so 43 -> 22 -> 11 values remain per lane before the in-row butterfly (66 swaps + 88 shuffles + 77 adds
// instead of 516 shuffles + 258 adds per item).  This tree defines the bits of a row: every item body stores its rows through it.
// AGENT: write-through (sc1) 8-byte stores -- the row's reader (the pair's updater) is another workgroup of the same launch, maybe on another XCD.
template <bool AGENT>
__device__ __forceinline__ void wave_row_store(const double row[43], double* P, const unsigned nhits, const int lane) {
  typedef unsigned int u2v __attribute__((ext_vector_type(2)));
  double P1[22], P2[11];
#pragma unroll
  for (int i = 0; i < 22; i++) {
    const double a = row[i], b2 = (i + 22 < 43) ? row[i + 22] : 0.0;
    const u2v lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b2), false, false);
    const u2v hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b2), false, false);
    // lanes 0..31: value i of lanes L and L+32;  lanes 32..63: value i+22 of lanes L-32 and L
    P1[i] = __hiloint2double((int)hi.x, (int)lo.x) + __hiloint2double((int)hi.y, (int)lo.y);
  }
#pragma unroll
  for (int i = 0; i < 11; i++) {
    const double a = P1[i], b2 = P1[i + 11];
    const u2v lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b2), false, false);
    const u2v hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b2), false, false);
    // even rows: P1[i] of rows r and r+1;  odd rows: P1[i+11] of rows r-1 and r
    double v = __hiloint2double((int)hi.x, (int)lo.x) + __hiloint2double((int)hi.y, (int)lo.y);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    P2[i] = v;
  }
  if ((lane & 15) == 0) {
    // row 0 (lane 0) holds values 0..10, row 1: 11..21, row 2: 22..32, row 3: 33..42 (+ the pad)
    const int row4 = lane >> 4, base = 11 * (row4 & 1) + 22 * (row4 >> 1);
    if (AGENT) {
      gu64* PG = (gu64*)reinterpret_cast<unsigned long long*>(P);
#pragma unroll
      for (int i = 0; i < 11; i++) if (base + i < 43) __hip_atomic_store(PG + base + i, (unsigned long long)__double_as_longlong(P2[i]), RLX_AGENT);
      if (lane == 0) __hip_atomic_store(PG + 43, (unsigned long long)__double_as_longlong((double)nhits), RLX_AGENT);
    } else {
#pragma unroll
      for (int i = 0; i < 11; i++) if (base + i < 43) P[base + i] = P2[i];
      if (lane == 0) P[43] = (double)nhits;
    }
  }
}

// ---- phase A, per point: the pieces every item body shares
// One axis of the moved point -- PCL 1.8 transformPointCloud scalar form (row `Ta` of T) -- and of the Jacobian point r = R x (row `Ra` of Rj;
// impl2:507-508).  Per axis, scalar outputs: the callers' unrolled loops then compile exactly as when the two lines stood in them.
__device__ __forceinline__ void move_axis(const float* Ta, const float* Ra, const float px, const float py, const float pz, float& xt, float& r) {
  xt = ((Ta[0] * px + Ta[1] * py) + Ta[2] * pz) + Ta[3];
  r = (Ra[0] * px + Ra[1] * py) + Ra[2] * pz;
}
// ... both are staged (six floats) for phase B
__device__ __forceinline__ void stage_point(float* sp, const float xt[3], const float r[3]) {
  sp[0] = xt[0]; sp[1] = xt[1]; sp[2] = xt[2]; sp[3] = r[0]; sp[4] = r[1]; sp[5] = r[2];
}
// getNeighborhoodAtPoint (voxel_grid_covariance_omp_impl.hpp:379-399): cell of the moved point, f32 divide (x / 2^k is the same bits as
// x * 2^-k, so a power-of-two leaf takes the one-instruction path), relative to the grid's min_b: "inside the grid" (impl:382-392) is then
// one unsigned compare per axis.
// (Measured: with this helper in sweep_item the tolerance arithmetic's one-launch align is 0.55-0.8 % slower than with the four lines written
//  out; the per-axis shape that cures it costs the exact DIRECT7 headline 0.4 %.  docs/experiments.md 10i has the numbers and the decision.)
__device__ __forceinline__ void rel_cell(const float xt[3], const SweepConst& sc, const float leaf, const int mb0, const int mb1, const int mb2,
                                         int& r0, int& r1, int& r2) {
  const int c0 = (int)floorf(sc.leaf_pow2 ? xt[0] * sc.inv_leaf : xt[0] / leaf);
  const int c1 = (int)floorf(sc.leaf_pow2 ? xt[1] * sc.inv_leaf : xt[1] / leaf);
  const int c2 = (int)floorf(sc.leaf_pow2 ? xt[2] * sc.inv_leaf : xt[2] / leaf);
  r0 = c0 - mb0; r1 = c1 - mb1; r2 = c2 - mb2;
}
// A probed bitmap word (bits lo, bits hi, prefix, pad) and the cell it was read for -> is the cell occupied, and its rank among the
// searchable leaves = voxel id.  Shift the cell's bit to the top: sign = occupied, popcount = bits at or below it.
__device__ __forceinline__ bool bitmap_rank(const uint4 bw, const unsigned cell, unsigned& id) {
  const unsigned long long bits = ((unsigned long long)bw.y << 32) | bw.x;
  const unsigned long long tb = bits << (63u - (cell & 63u));
  id = bw.z + (unsigned)__popcll(tb) - 1u;
  return (long long)tb < 0;
}

// The LDS of a work item by purpose (SLOT) and shape, declared outside the item functions: a function's own __shared__ arrays are one set per
// instantiation, and the score-only and the full item body of one kernel (SO) must share theirs, not each take the workgroup's LDS.
template <typename T, int SLOT>
__device__ __forceinline__ T& item_lds() { __shared__ T v; return v; }

// ---- phase B: the wave's hit queue, its 64-hit batches and the lane sums they go into.  One definition for every item body: which hits
// form a batch, and in which order a lane adds them, is part of a row's bits.
// One batch of queued hits (one per lane): queue entry + the voxel record it points at, in registers.
struct BatchX { unsigned slot; double m0, m1, m2; float C[9]; int weight; double w; };
struct BatchF { unsigned slot; float mh[3], ml[3], c[6]; int weight; float w; };
struct BatchD { unsigned slot; double m0, m1, m2; double C[9]; };            // PM = 2: the f64 mean and the f64 inverse covariance
// `ent` / `qw` / `stage`: the wave's rows of the LDS queue (Q_CAP entries, a power of two), of its ndt_pca weights and of its staged points.
// SO: hits are evaluated by eval_score / eval_score_fast (acc[0] alone).
// W_LATE (ndt_pca, K = 1: the hit's weight is the leaf's own, read with its record): widen it when the batch is evaluated, not when it is
// fetched -- the same value either way, but two registers fewer across the mid-evaluation prefetch.  sweep_rows_d1 needs that (with the
// widening at the fetch the pca / DIRECT1 headline lost 5 %, docs/experiments.md 10i); sweep_item widens at the fetch as it always did.
// PM (MI355NDT_OPT_POSE_MODEL): 1 = hits are evaluated by eval_hit_euler -- the staged point's second half is the ORIGINAL point and `rw` the pair's
// 23 rows (set by the item body; no member at all for PM = 0, whose kernels keep their register tables).
// PM = 2 (MI355NDT_OPT_NDT_CLASS = 1, K = 27 alone): hits are evaluated by eval_hit_pcl -- the staged points as for PM = 1, `rw` the pair's rows as
// doubles and the grid's f64 inverse covariances, which a batch fetches in place of the record's f32 ones.
// GATE (MI355NDT_OPT_GROUND_CLASS = 1 / 2, pclomp_ground's per-point gate): the probe stage has decided already which points' hits enter the
// queue and has kept dead leaves out of it (sweep_item), so every queued hit is evaluated as ndt_omp's.  The tag changes nothing in here; it
// states which instantiations exist.
struct NoRows {};
template <bool PCA, int K, int ORD, bool SO, int Q_CAP, bool W_LATE = false, int PM = 0, bool LEAN = false, bool GATE = false>
struct HitQueue {
  static_assert(!GATE || (!PCA && PM == 0 && ORD != 2 && !SO && !LEAN && !W_LATE && (K == 1 || K == 7 || K == 26)), "the gated sweep: ndt_omp, DIRECT searches, exact arithmetic, full rows");
  static_assert(PM == 0 || ((PM == 1 || PM == 2) && !PCA && ORD != 2 && !SO), "the Euler model: ndt_omp, exact arithmetic, full rows");
  static_assert(PM != 2 || (K == 27 && ORD == 0), "PCL's class: the radius search, one instantiation");
  typename std::conditional<PM == 1, EulerRows, typename std::conditional<PM == 2, PclCtx, NoRows>::type>::type rw;
  static constexpr bool KD = (K == 27), FAST = (ORD == 2), PCAQ = PCA && K > 1;
  static constexpr int NA = FAST ? NACC_F : 43;
  typedef typename std::conditional<FAST, float, double>::type AccT;
  // ndt_pca weight of a queued hit: the suffix product (f64: up to ~150^7) -- for DIRECT1 just the leaf's own integer weight
  typedef typename std::conditional<K == 1, int, AccT>::type QW;
  typedef typename std::conditional<FAST, BatchF, typename std::conditional<PM == 2, BatchD, BatchX>::type>::type Batch;
  unsigned* const ent; QW* const qw; const float (*const stage)[6];
  const VoxelRec* const R; const SweepConst& sc; const double* const exp_tab;
  const int lane; const unsigned long long lt_mask;
  // The lane sums of the row being built.  The item body declares the array and reads it back as Q.acc; the queue zeroes it (new_row) and adds
  // into it.  The split is the register allocator's: with the array as a member here k_sweep<true, 7, 1, true, .> has one VGPR fewer than
  // before the queue had a definition of its own, and kernels are held to their old register tables (docs/experiments.md 10i).
  AccT (&acc)[NA];
  unsigned nhits;                                  // wave-uniform
  int head, count;                                 // wave-uniform
  int old;                                         // queued entries that reference the OTHER staging half (older super-tile; sweep_item)
  __device__ __forceinline__ HitQueue(AccT (&acc_)[NA], unsigned* ent_, QW* qw_, const float (*stage_)[6], const VoxelRec* R_, const SweepConst& sc_, const double* exp_tab_, const int lane_)
      : ent(ent_), qw(qw_), stage(stage_), R(R_), sc(sc_), exp_tab(exp_tab_), lane(lane_), lt_mask((1ull << lane_) - 1ull), acc(acc_), head(0), count(0), old(0) { new_row(); }
  __device__ __forceinline__ void new_row() {
#pragma unroll
    for (int a = 0; a < NA; a++) acc[a] = (AccT)0;
    nhits = 0;
  }
  // the lanes with `hit` append (staging slot, voxel id) -- ballot + popcount compaction, lane order -- and, ndt_pca with K > 1, the weight
  __device__ __forceinline__ void push(const bool hit, const unsigned slot, const unsigned id, const double w) {
    const unsigned long long mask = __ballot(hit);
    if (hit) {
      const int pos = (head + count + (int)__popcll(mask & lt_mask)) & (Q_CAP - 1);
      ent[pos] = (slot << ID_BITS) | id;
      if (PCAQ) qw[pos] = (QW)w;
    }
    count += (int)__popcll(mask);
  }
  // read the `m` hits that sit `off` entries behind the queue head; lanes >= m re-read the last entry (and contribute +0)
  __device__ __forceinline__ void fetch(const int off, const int m, Batch& B) const {
    const int k = lane < m ? lane : m - 1;
    const unsigned e = ent[(head + off + k) & (Q_CAP - 1)];
    B.slot = e >> ID_BITS;
    if constexpr (FAST) {
      const VoxelRecF& vr = reinterpret_cast<const VoxelRecF*>(R)[e & ((1u << ID_BITS) - 1)];
#pragma unroll
      for (int a = 0; a < 3; a++) { B.mh[a] = vr.mh[a]; B.ml[a] = vr.ml[a]; }
#pragma unroll
      for (int a = 0; a < 6; a++) B.c[a] = vr.c[a];
      B.weight = vr.weight;
      if (!W_LATE) B.w = 1.f;
      if (PCAQ) B.w = (float)qw[(head + off + k) & (Q_CAP - 1)];
      else if (PCA && !W_LATE) B.w = (float)vr.weight;
    } else if constexpr (PM == 2) {
      const unsigned id = e & ((1u << ID_BITS) - 1);
      const VoxelRec& vr = R[id];
      B.m0 = vr.mean[0]; B.m1 = vr.mean[1]; B.m2 = vr.mean[2];
#pragma unroll
      for (int a = 0; a < 9; a++) B.C[a] = rw.icov64[(size_t)id * 9 + a];
    } else {
      const VoxelRec& vr = R[e & ((1u << ID_BITS) - 1)];
      B.m0 = vr.mean[0]; B.m1 = vr.mean[1]; B.m2 = vr.mean[2];
#pragma unroll
      for (int a = 0; a < 9; a++) B.C[a] = vr.icov[a];
      B.weight = vr.weight;
      if (!W_LATE) B.w = 1.0;
      if (PCAQ) B.w = (double)qw[(head + off + k) & (Q_CAP - 1)];
      else if (PCA && !W_LATE) B.w = (double)vr.weight;
    }
  }
  // evaluate a fetched batch (running `mid` half way through) and retire its `m` queue entries
  template <typename Mid>
  __device__ __forceinline__ void eval_batch(const Batch& B, const int m, Mid mid) {
    const float* sp = stage[B.slot];               // staged point: LDS, short latency
    const float xt0 = sp[0], xt1 = sp[1], xt2 = sp[2];
    float r[3] = {sp[3], sp[4], sp[5]};
    // ndt_omp: leaves with nr_points = -1 (eigen / inverse failure) are not neighbours (impl:395): filtered here
    bool live = lane < m;
    if constexpr (PM != 2) live = live && (PCAQ || KD || B.weight != VOX_DEAD);
    if constexpr (PM == 2) {
      const double u[3] = {(double)xt0 - B.m0, (double)xt1 - B.m1, (double)xt2 - B.m2};
      eval_hit_pcl<Mid>(u, r, B.C, rw.rows, sc.d1, sc.d2, live, acc, mid);
    } else if constexpr (FAST) {
      float u[3] = {(xt0 - B.mh[0]) - B.ml[0], (xt1 - B.mh[1]) - B.ml[1], (xt2 - B.mh[2]) - B.ml[2]};
      const float w = (W_LATE && !PCAQ) ? (PCA ? (float)B.weight : 1.f) : B.w;
      if constexpr (SO) { mid(); eval_score_fast<PCA>(u, B.c, sc.d1f, sc.d2f, sc.kq, w, live, acc[0]); }
      else eval_hit_fast<PCA, Mid>(u, r, B.c, sc.d1f, sc.d2f, sc.kq, w, live, acc, mid);
    } else {
      float u[3] = {(float)((double)xt0 - B.m0), (float)((double)xt1 - B.m1), (float)((double)xt2 - B.m2)};   // impl2:276-279, 574
      const double w = (W_LATE && !PCAQ) ? (PCA ? (double)B.weight : 1.0) : B.w;
      if constexpr (SO) { mid(); eval_score<PCA, ORD>(u, B.C, sc.d1, sc.d2f, w, live, acc[0], exp_tab); }
      else if constexpr (PM == 1) eval_hit_euler<Mid, KD, ORD>(u, r, B.C, rw, sc.d1, sc.d2f, live, acc, exp_tab, mid);
      else eval_hit<PCA, Mid, KD, ORD>(u, r, B.C, sc.d1, sc.d2f, w, live, acc, exp_tab, mid);
    }
    nhits += PCAQ ? (unsigned)m : (unsigned)__popcll(__ballot(live));
    head = (head + m) & (Q_CAP - 1);
    count -= m;
    old = old > m ? old - m : 0;
  }
  // evaluate `m` queued hits (m <= 64), one per lane
  __device__ __forceinline__ void drain(const int m) {
    Batch B;
    fetch(0, m, B);
    eval_batch(B, m, NoHook());
  }
  // All full batches in the queue, software-pipelined: the next batch's record loads are issued in the middle of the
  // current batch's arithmetic (before its 36 Hessian terms), so their L2 latency is off the critical path.
  __device__ __forceinline__ void drain_full() {
    // (PM = 2: the f64 evaluation is bound by its arithmetic, and the 25 registers of a second batch in flight are the ones it would spill)
    if (PM == 2 || !SweepTune<PCA, K, ORD, LEAN>::PIPE) {           // plain: one batch after the other
      while (count >= 64) drain(64);
      return;
    }
    if (count < 64) return;
    Batch A;
    fetch(0, 64, A);
#pragma unroll 1
    for (;;) {
      const bool more = count >= 128;
      Batch N;
      eval_batch(A, 64, [&]() { if (more) fetch(64, 64, N); });
      if (!more) break;
      A = N;
    }
  }
};

// SO: score-only item (the pair's last sweep, PairState::last_sweep): the same probe stage, hit queue, 64-hit batches and ndt_pca weights; each
// hit is evaluated by eval_score / eval_score_fast and the row carries the score and the hit count alone (the one-launch align, and
// k_pose_scores of ndt_pose_scores.hpp, whose items are nothing else).
// PM = 1 (MI355NDT_OPT_POSE_MODEL, the lockstep rounds only): phase A stages the moved point and the ORIGINAL point, phase B is eval_hit_euler over
// the pair's rows sc.euler_rows[b] (written by whoever wrote the pair's T: k_init_state, k_set_pose_p, newton_update).
// GATE (MI355NDT_OPT_GROUND_CLASS = 1 / 2, the lockstep rounds only): computeDerivatives_seg (ndt_ground_impl.hpp:484-546) adds a point's sums
// only if the class of the LAST neighbour the search returned is the wanted one.  Probes run last to first here, so the first live neighbour the
// probe stage meets is that one: its class code (sc.leaf_class, a byte per record, loaded where ndt_pca loads its weights) fixes the point's
// verdict, and the point's hits are pushed only if it is sc.gate_code.  A leaf with code 0 (nr_points == -1) is no neighbour (impl:395) and
// neither decides nor enters the queue.  A point without a live neighbour pushes nothing -- what both classes add for it.
template <bool PCA, int K, int IT, bool FINE, int ORD, bool ASYNC, bool SO = false, int PM = 0, bool LEAN = false, bool GATE = false>
__device__ __forceinline__ void sweep_item(const int b, const int rem, const float* __restrict__ src, const size_t pitch, const PairState* st,
                                           const GridDesc* __restrict__ gd, const BitWord* __restrict__ words, const VoxelRec* __restrict__ recs,
                                           double* partials, const int rows_per_pair, const SweepConst& sc, const float* __restrict__ cent,
                                           const int* __restrict__ grid_of, const double* exp_tab,
                                           const unsigned pose_w, const int n_async, const int g_async,  /* ASYNC only: pose words (sweep_pose_words), point count, grid index */
                                           Timeline& tl) {
  constexpr bool KD = (K == 27);
  constexpr bool FAST = (ORD == 2);                // tolerance arithmetic (eval_hit_fast): `recs` holds VoxelRecF records
  static_assert(!SO || (ASYNC && !FINE), "score-only items: the one-launch align's last sweep and the pose scores (ndt_pose_scores.hpp), both with the pose in words");
  static_assert(!FAST || K == 1 || K == 7, "tolerance arithmetic is instantiated for DIRECT1 / DIRECT7");
  static_assert(PM == 0 || (!PCA && !FAST && !ASYNC && !FINE && !SO), "the Euler model takes the lockstep rounds: ndt_omp, exact arithmetic, batch items");
  static_assert(PM != 2 || (K == 27 && ORD == 0 && IT == 8), "PCL's class: the radius search, batch items");
  static_assert(!LEAN || (ASYNC && !FINE && PM == 0 && IT == 8), "the lean body belongs to the one-launch align");
  static_assert(!GATE || (!PCA && !FAST && !ASYNC && !FINE && !SO && PM == 0 && IT == 8 && (K == 1 || K == 7 || K == 26)), "the gated sweep takes the lockstep rounds: ndt_omp, DIRECT searches, exact arithmetic, batch items");
  typedef SweepTune<PCA, K, ORD, LEAN> Tune;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // ndt_pca's per-hit multiplier is the product of the hit's own weight and those of the point's LATER hits, known only in phase A.
  // With one probe per point (DIRECT1) it is just the leaf's own weight, which phase B reads with the record anyway: no weight
  // load in the probe stage, no weight queue, dead leaves filtered in phase B exactly as for ndt_omp.
  constexpr bool PCAQ = PCA && K > 1;
  // per-wave hit queue: must hold a leftover (< 64) plus everything one probe group can push: TP tiles x min(K, Q_GROUP) probes x 64
  constexpr int TPS = Tune::TP < IT ? Tune::TP : IT;         // tiles of a super-tile: the staging geometry and the partial drains
  constexpr int TP = Tune::TPP < TPS ? Tune::TPP : TPS;      // tiles of a probe group (= the super-tile, except in the lean body)
  constexpr int GPS = TPS / TP;                              // probe groups per super-tile
  static_assert(TPS % TP == 0, "probe groups tile the super-tile");
  constexpr int Q_NEED = (IT / TP > 1 ? 64 : 0) + TP * (K < Q_GROUP ? K : Q_GROUP) * 64;
  constexpr int Q_CAP = FAST ? (Q_NEED <= 128 ? 128 : Q_NEED <= 256 ? 256 : Q_NEED <= 512 ? 512 : 1024) : ((K > 1 && K <= Q_GROUP) ? 1024 : 512);
  static_assert(Q_NEED <= Q_CAP, "hit queue");
  typedef HitQueue<PCA, K, ORD, SO, Q_CAP, false, PM, LEAN, GATE> Queue;
  auto& q_ent = item_lds<unsigned[WAVES][Q_CAP], 0>();
  auto& q_w = item_lds<typename Queue::QW[PCAQ ? WAVES : 1][PCAQ ? Q_CAP : 1], 1>();
  // TP tiles of 64 points are probed together ("super-tile"): their point transforms, then ALL their bitmap loads, then all
  // their ballots -- the probe stage costs a few L2 round trips per super-tile, not per tile.  DIRECT1 has one probe per point
  // and ~0.9 hits, so it is probe-stage bound: 4 tiles at a time; DIRECT7: 2 (14 bitmap words in flight); the 26/27-cell
  // searches already have 7-probe groups inside one tile.
  // The lean body probes ONE tile at a time and keeps everything else of the two-tile super-tile: the staging halves, and the boundaries at
  // which the entries of the older half are drained.
  constexpr int NBUF = (IT / TPS > 1) ? 2 : 1;   // a super-tile that is the whole item needs no second buffer
  auto& stage = item_lds<float[WAVES][NBUF * 64 * TPS][6], 2>();   // (two) super-tiles of staged points: x'(3), R x (3)

  // FINE: the four waves of a block always hold the four rows of ONE chunk (items 4q .. 4q+3: static dealing, four waves per block, a
  // multiple of four items per pair), so the chunk level of k_update's tree -- ((r0 + r1) + r2) + r3 -- is added here through LDS and
  // one row per chunk goes to memory: a quarter of the rows for the update to fetch.
  auto& red = item_lds<double[FINE ? WAVES : 1][FINE ? NACC : 1], 3>();
  const PairState& S = st[b];
  // ASYNC: T (12 words), Rj (9) and n_src through agent-scope vector loads (never the scalar cache, never a stale L1 line): the
  // updater of this pair -- some other workgroup of this launch -- rewrote them since the pair's previous sweep
  // (the caller issued that load -- sweep_pose_words -- as early as it knew the pair, so that it is in flight together with the point loads
  //  below; the point count comes from the batch's constant count array for the same reason)
  const int n = ASYNC ? n_async : S.n_src;
  const GridDesc& g = gd[ASYNC ? g_async : (grid_of ? grid_of[b] : b)];
  const float* X = src + (size_t)b * 3 * pitch;
  const BitWord* W = words + g.word_off;
  const VoxelRec* R = recs + g.rec_off;
  const unsigned char* LC = nullptr;                                           // GATE: the class codes of this grid's records
  if constexpr (GATE) LC = sc.leaf_class + g.rec_off;
  const bool grid_ok = (g.status == GRID_OK);
  float T[12], Rj[9];
  if constexpr (ASYNC) pose_from_words(pose_w, T, Rj);
  else {
#pragma unroll
    for (int a = 0; a < 12; a++) T[a] = S.T[a];
#pragma unroll
    for (int a = 0; a < 9; a++) Rj[a] = PM != 0 ? 0.f : S.Rj[a];               // (PM = 1: no Jacobian point, Rj is not read)
  }
  const float leaf = g.leaf;
  const int mb0 = g.min_b[0], mb1 = g.min_b[1], mb2 = g.min_b[2];
  const int xb0 = g.max_b[0], xb1 = g.max_b[1], xb2 = g.max_b[2];
  const int mul1 = g.mul1, mul2 = g.mul2, nwords = g.nwords;
  {
    typename Queue::AccT acc[Queue::NA];
    Queue Q(acc, q_ent[wv], q_w[PCAQ ? wv : 0], stage[wv], R, sc, exp_tab, lane);
    // a work item belongs to one pair: a wave-uniform index, so the 69 floats come through the scalar cache
    if constexpr (PM == 1) Q.rw = euler_rows_of_pair(sc.euler_rows, b);
    // (PM = 2: 69 doubles, too many to sit in scalar registers at once -- each is loaded where its operation needs it)
    if constexpr (PM == 2) { Q.rw.rows = pcl_rows_of_pair(sc.pcl_rows, b); Q.rw.icov64 = sc.icov64 + (size_t)g.rec_off * 9; }
    const int wbase = rem * (IT * 64);
    if (wbase < n && grid_ok) {
      constexpr int NST = IT / TP;                            // probe groups per item (= super-tiles, except in the lean body)
      const unsigned e0 = (unsigned)(xb0 - mb0), e1 = (unsigned)(xb1 - mb1), e2 = (unsigned)(xb2 - mb2);
      const unsigned empty_cell = (unsigned)(nwords - 1) << 6;
      // points of the next super-tile are fetched one super-tile ahead (HBM latency ~2 us would otherwise be exposed each time)
      float nx[TP], ny[TP], nz[TP];
#pragma unroll
      for (int p = 0; p < TP; p++) {
        const int i = wbase + p * 64 + lane;
        nx[p] = ny[p] = nz[p] = 0.f;
        if (i < n) { nx[p] = X[i]; ny[p] = X[pitch + i]; nz[p] = X[2 * pitch + i]; }
      }
      TL_STAMP(1);
#pragma unroll 1
      for (int st = 0; st < NST; st++) {
        if (wbase + st * TP * 64 >= n) break;        // wave-uniform
        // the staging area holds two super-tiles: entries of super-tile st-2 must be gone before st overwrites their half
        // (only happens when hits are sparse; dense tiles are consumed by the regular 64-wide drains)
        if (GPS == 1 || st % GPS == 0) {             // (a super-tile begins: always, except in the lean body)
          if (Q.old > 0) { __builtin_amdgcn_wave_barrier(); Q.drain(Q.old); }
          Q.old = Q.count;
        }
        // staging tile of tile p of this probe group: the super-tile's half, the group's place in it
#define NDT_STAGE_TILE(p) (GPS == 1 ? (st & 1) * TP + (p) : ((st / GPS) & 1) * TPS + (st % GPS) * TP + (p))
        int r0[TP], r1[TP], r2[TP], cc[TP];
        bool valid[TP];
        float kx[TP], ky[TP], kz[TP];                // moved points (only the KDTREE distance test reads them again)
#pragma unroll
        for (int p = 0; p < TP; p++) {
          const int i = wbase + (st * TP + p) * 64 + lane;
          const float px = nx[p], py = ny[p], pz = nz[p];
          const int inext = i + TP * 64;
          if (st + 1 < NST && inext < n) { nx[p] = X[inext]; ny[p] = X[pitch + inext]; nz[p] = X[2 * pitch + inext]; }
          bool ok = i < n && finite3(px, py, pz);
          float xt[3], r[3];
#pragma unroll
          for (int a = 0; a < 3; a++) move_axis(T + 4 * a, Rj + 3 * a, px, py, pz, xt[a], r[a]);
          // a non-finite moved point (NaN pose: only reachable through a NaN More-Thuente trial value) has no neighbours;
          // the reference's float->int cast is undefined there
          ok = ok && finite3(xt[0], xt[1], xt[2]);
          if constexpr (PM != 0) { const float xo[3] = {px, py, pz}; stage_point(stage[wv][NDT_STAGE_TILE(p) * 64 + lane], xt, xo); }
          else stage_point(stage[wv][NDT_STAGE_TILE(p) * 64 + lane], xt, r);
          kx[p] = xt[0]; ky[p] = xt[1]; kz[p] = xt[2];
          // Branch-free probe stage.  Relative cell r = c - min_b; "inside the grid" (impl:382-392) is one unsigned
          // compare per axis; a probe that falls outside (or belongs to an invalid lane) is redirected to the grid's
          // spare all-zero bitmap word, so it misses without any flag having to be kept.
          rel_cell(xt, sc, leaf, mb0, mb1, mb2, r0[p], r1[p], r2[p]);
          cc[p] = r0[p] + r1[p] * mul1 + r2[p] * mul2;
          valid[p] = ok;
        }
        // probes run last-to-first so the ndt_pca weight of a hit (product of its own and all LATER hits' weights,
        // ndt_pca_impl2.hpp:295-296) is a running product; the order of the f64 additions is free anyway.
        TL_STAMP(2);
        double suf[TP];
#pragma unroll
        for (int p = 0; p < TP; p++) suf[p] = 1.0;
        int verdict[TP];                             // GATE: the class code of the point's deciding neighbour (0: none met yet)
#pragma unroll
        for (int p = 0; p < TP; p++) verdict[p] = LEAF_CLASS_NONE;
        // Q_GROUP probes of every tile of the super-tile at a time: all their bitmap loads in flight together (then all
        // ndt_pca weight loads), then the ballots -- one L2 round trip per stage.
#pragma unroll
        for (int q1 = K; q1 > 0; q1 -= Q_GROUP) {      // compile-time groups: 1 for DIRECT1 / DIRECT7, 4 for DIRECT26 / KDTREE
          unsigned cellv[TP][Q_GROUP];
          uint4 bwv[TP][Q_GROUP];                      // BitWord: bits lo, bits hi, prefix, pad
#pragma unroll
          for (int p = 0; p < TP; p++) {
#pragma unroll
            for (int j = 0; j < Q_GROUP; j++) {
              const int q = q1 - 1 - j;               // compile-time
              if (q < 0) continue;
              const int o0 = probe_off(K, q, 0), o1 = probe_off(K, q, 1), o2 = probe_off(K, q, 2);
              const bool inside = valid[p] && (unsigned)(r0[p] + o0) <= e0 && (unsigned)(r1[p] + o1) <= e1 && (unsigned)(r2[p] + o2) <= e2;
              cellv[p][j] = inside ? (unsigned)(cc[p] + o0 + o1 * mul1 + o2 * mul2) : empty_cell;
              bwv[p][j] = *reinterpret_cast<const uint4*>(W + (cellv[p][j] >> 6));
            }
          }
          TL_STAMP(3);
          unsigned idv[TP][Q_GROUP];
          int wiv[TP][Q_GROUP];
#pragma unroll
          for (int p = 0; p < TP; p++) {
#pragma unroll
            for (int j = 0; j < Q_GROUP; j++) {
              if (q1 - 1 - j < 0) continue;
              // occupied cells alone are hits; ndt_pca needs the weights now (suffix product), ndt_omp filters dead leaves in phase B
              // instead and saves this dependent L2 round trip
              const bool occ = bitmap_rank(bwv[p][j], cellv[p][j], idv[p][j]);
              wiv[p][j] = occ ? 1 : VOX_DEAD;
              if (PCAQ) { if (occ) wiv[p][j] = R[idv[p][j]].weight; }
              // the gate needs the leaf's class now; code 0 = a dead leaf, which phase B would filter too late to keep it from deciding
              if constexpr (GATE) { if (occ) { const int code = (int)LC[idv[p][j]]; wiv[p][j] = code == LEAF_CLASS_NONE ? VOX_DEAD : code; } }
              if (KD && occ) {                     // FLANN L2_Simple distance to the leaf's f32 centroid
                const float* cp = cent + 3 * (size_t)(g.rec_off + idv[p][j]);
                const float dx = kx[p] - cp[0], dy = ky[p] - cp[1], dz = kz[p] - cp[2];
                if (!(((dx * dx + dy * dy) + dz * dz) < sc.kd_r2)) wiv[p][j] = VOX_DEAD;
              }
            }
          }
#pragma unroll
          for (int p = 0; p < TP; p++) {
            const int slot = NDT_STAGE_TILE(p) * 64 + lane;
#pragma unroll
            for (int j = 0; j < Q_GROUP; j++) {
              if (q1 - 1 - j < 0) continue;
              bool hit = wiv[p][j] != VOX_DEAD;           // empty cell, or nr_points == -1: not a neighbour (impl:395)
              if constexpr (GATE) {                       // the first live neighbour met = the reference's last one: its class is the point's
                if (hit && verdict[p] == LEAF_CLASS_NONE) verdict[p] = wiv[p][j];
                hit = hit && verdict[p] == sc.gate_code;
              }
              if (PCAQ && hit) suf[p] *= (double)wiv[p][j];
              Q.push(hit, (unsigned)slot, idv[p][j], suf[p]);
            }
          }
          __builtin_amdgcn_wave_barrier();
          TL_STAMP(4);
          Q.drain_full();
          TL_STAMP(5);
        }
      }
#undef NDT_STAGE_TILE
      __builtin_amdgcn_wave_barrier();
      if (Q.count > 0) Q.drain(Q.count);
      TL_STAMP(5);
    }
    // one row per (chunk, quarter); FINE: into the block's LDS first (below)
    double* P = FINE ? &red[FINE ? wv : 0][0] : partials + ((size_t)b * rows_per_pair + rem) * NACC;
    if constexpr (SO) score_row_store((double)Q.acc[0], P, Q.nhits, lane);
    else if constexpr (FAST) {
      double accd[43];
      fast_acc_to_row(Q.acc, accd);
      wave_row_store<ASYNC && !FINE>(accd, P, Q.nhits, lane);
    } else wave_row_store<ASYNC && !FINE>(Q.acc, P, Q.nhits, lane);
    if (FINE) {
      __syncthreads();                              // (uniform: the four waves of a block run the same items loop, see above)
      if (wv == 0 && lane < NACC)
        partials[((size_t)b * (rows_per_pair >> 2) + (rem >> 2)) * NACC + lane] = ((red[0][lane] + red[FINE ? 1 : 0][lane]) + red[FINE ? 2 : 0][lane]) + red[FINE ? 3 : 0][lane];
      __syncthreads();
    }
    TL_STAMP(6);
    tl.count();
  }
}

// DIRECT1 in the one-launch align: NROWS consecutive work items of ONE pair (the two items of a claim, ndt_async.hpp) as one software
// pipeline.  With one probe per point and ~0.85 hits, a DIRECT1 item is a third evaluation and two thirds waiting for the chain
// points -> bitmap word -> record (timeline build, pca / 1 m: point wait + transform 11 %, bitmap wait + push 18 %, reduction 10 % of an item).
// sweep_item probes the whole item at once -- every wait of that chain is exposed once per item.  Here a row's eight tiles go through in four
// super-tiles of two: while super-tile s is evaluated, the bitmap words of s + 1 and the points of s + 2 are in flight, and the first
// super-tile of the NEXT row is probed under this row's reduction.  What is evaluated, and in which 64-hit batches, is exactly what
// sweep_item<PCA, 1, 8> does -- hits enter the queue in point order, full batches leave it in FIFO order, the tail is flushed at the end of
// every row -- so the rows carry the same bits (tests/test_gpu_configs.py and tests/test_stream_gpu.py hold this function, which the
// one-launch align uses, against the round-based kernels, which use sweep_item).
// The staging area holds one row (four super-tiles); a super-tile's slot is free again when its row has been flushed.
// SO: score-only rows (the pair's last sweep), as sweep_item's SO.
template <bool PCA, int ORD, int NROWS, bool SO = false>
__device__ __forceinline__ void sweep_rows_d1(const int b, const int rem0, const float* __restrict__ src, const size_t pitch,
                                              const GridDesc* __restrict__ gd, const BitWord* __restrict__ words, const VoxelRec* __restrict__ recs,
                                              double* partials, const int rows_per_pair, const SweepConst& sc, const double* exp_tab,
                                              const unsigned pose_w, const int n, const int g_idx, Timeline& tl) {
  constexpr int TP = 2, IT = 8, NST = IT / TP, Q_CAP = 512;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  auto& q_ent = item_lds<unsigned[WAVES][Q_CAP], 4>();
  auto& stage = item_lds<float[WAVES][64 * IT][6], 5>();   // one row of staged points: x'(3), R x (3)
  const GridDesc& g = gd[g_idx];
  const float* X = src + (size_t)b * 3 * pitch;
  const BitWord* W = words + g.word_off;
  const VoxelRec* R = recs + g.rec_off;
  const bool grid_ok = (g.status == GRID_OK);
  float T[12], Rj[9];
  pose_from_words(pose_w, T, Rj);
  const float leaf = g.leaf;
  const int mb0 = g.min_b[0], mb1 = g.min_b[1], mb2 = g.min_b[2];
  const unsigned e0 = (unsigned)(g.max_b[0] - mb0), e1 = (unsigned)(g.max_b[1] - mb1), e2 = (unsigned)(g.max_b[2] - mb2);
  const int mul1 = g.mul1, mul2 = g.mul2;
  const int base = rem0 * (IT * 64);               // first point of the first row
  constexpr int S_TOTAL = NROWS * NST;

  // sweep_item<PCA, 1, 8>'s queue: one probe per point, exact arithmetic, the leaf's own weight read with its record (no weight queue)
  double acc[43];
  HitQueue<PCA, 1, ORD, SO, Q_CAP, true> Q(acc, q_ent[wv], nullptr, stage[wv], R, sc, exp_tab, lane);

  // pipeline registers: points of the super-tile after the probed one; probe words of the probed one
  float nx[TP], ny[TP], nz[TP];
  uint4 bw[TP];
  unsigned cellv[TP];
  auto load_points = [&](const int s) {
#pragma unroll
    for (int p = 0; p < TP; p++) {
      const int i = base + (s * TP + p) * 64 + lane;
      nx[p] = ny[p] = nz[p] = 0.f;
      if (s < S_TOTAL && i < n) { nx[p] = X[i]; ny[p] = X[pitch + i]; nz[p] = X[2 * pitch + i]; }
    }
  };
  // transform super-tile s (its points are in nx..), stage it, and issue its bitmap loads
  auto probe = [&](const int s) {
#pragma unroll
    for (int p = 0; p < TP; p++) {
      const int i = base + (s * TP + p) * 64 + lane;
      const float px = nx[p], py = ny[p], pz = nz[p];
      bool ok = grid_ok && i < n && finite3(px, py, pz);
      float xt[3], r[3];
#pragma unroll
      for (int a = 0; a < 3; a++) move_axis(T + 4 * a, Rj + 3 * a, px, py, pz, xt[a], r[a]);
      ok = ok && finite3(xt[0], xt[1], xt[2]);
      stage_point(stage[wv][(((s % NST) * TP) + p) * 64 + lane], xt, r);
      int r0, r1, r2;
      rel_cell(xt, sc, leaf, mb0, mb1, mb2, r0, r1, r2);
      const bool inside = ok && (unsigned)r0 <= e0 && (unsigned)r1 <= e1 && (unsigned)r2 <= e2;
      // (a probe that falls outside the grid -- or belongs to an invalid lane, or to a target without a grid -- reads nothing and misses)
      cellv[p] = inside ? (unsigned)(r0 + r1 * mul1 + r2 * mul2) : 0u;
      bw[p] = make_uint4(0u, 0u, 0u, 0u);
      if (inside) bw[p] = *reinterpret_cast<const uint4*>(W + (cellv[p] >> 6));
    }
  };
  // rank the probed super-tile's cells and push its hits (point order: tile, then lane)
  auto push = [&](const int s) {
#pragma unroll
    for (int p = 0; p < TP; p++) {
      unsigned id;
      const bool hit = bitmap_rank(bw[p], cellv[p], id);
      Q.push(hit, (unsigned)((((s % NST) * TP) + p) * 64 + lane), id, 1.0);
    }
    __builtin_amdgcn_wave_barrier();
  };

  load_points(0);
  TL_STAMP(1);
  probe(0);
  load_points(1);
  TL_STAMP(2);
#pragma unroll 1
  for (int s = 0; s < S_TOTAL; s++) {
    const bool row_end = (s % NST) == NST - 1;
    push(s);
    TL_STAMP(4);
    if (!row_end) { probe(s + 1); load_points(s + 2); }        // their memory round trips ride under the evaluation below
    Q.drain_full();
    TL_STAMP(5);
    if (!row_end) continue;
    // ---- the row is complete: flush the tail, then (the staging area is free) probe the next row's first super-tile under the reduction
    __builtin_amdgcn_wave_barrier();
    if (Q.count > 0) Q.drain(Q.count);
    TL_STAMP(5);
    if (s + 1 < S_TOTAL) { probe(s + 1); load_points(s + 2); }
    double* P = partials + ((size_t)b * rows_per_pair + rem0 + s / NST) * NACC;
    if constexpr (SO) score_row_store(Q.acc[0], P, Q.nhits, lane);
    else wave_row_store<true>(Q.acc, P, Q.nhits, lane);
    Q.new_row();
    TL_STAMP(6);
    tl.count();
  }
}

template <bool PCA, int K, int IT = 8, bool FINE = false, int ORD = 0, int PM = 0, bool GATE = false>
__global__ void __launch_bounds__(SWEEP_THREADS, (SweepTune<PCA, K, ORD>::WPE))
k_sweep(const float* __restrict__ src, size_t pitch, const PairState* __restrict__ st,
        const GridDesc* __restrict__ gd, const BitWord* __restrict__ words, const VoxelRec* __restrict__ recs,
        double* partials, int rows_per_pair, const int* __restrict__ active_list, SweepCtl* ctl, SweepCtl* ctl_next, SweepConst sc,
        const float* __restrict__ cent, const int* __restrict__ grid_of) {
  // K == 27 is the KDTREE mode (ndt_omp_impl2.hpp:251-253): radiusSearch(point, resolution) over the f32 centroids of the
  // searchable leaves (voxel_grid_covariance_omp.h:505-534).  A centroid lies inside its own cell, so every centroid closer
  // than one leaf sits in the 3x3x3 block around the point's cell: probe those 27 cells and keep d^2 < float(r*r).  The
  // reference does not re-check nr_points there, so eigen/inverse-failed leaves DO take part (their icov is zero / non-finite).
  // Persistent waves pulling work items.  One item = one wave-quarter (CHUNK_PTS/4 consecutive points) of one chunk
  // of one active pair; every wave is independent (own LDS queue, own partial row, no block barrier), so a wave
  // whose points have few hits simply takes the next item instead of idling at a barrier.
  // Items are queued per XCD: pair slot a of the active list belongs to XCD a % 8 (workgroup L is observed to run on
  // XCD L % 8, MI355X_MICROARCH.md), so one pair's records / bitmap / points stay in one L2; a wave whose XCD
  // queue is empty steals from the others.  Which wave runs an item never changes the item's result.
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_active = ctl->n_active;
  const int items_per_pair = rows_per_pair;         // one partial row per work item

  __shared__ double exp_tab[64];                   // 2^(j/64) for ndtm::exp_f32arg
  if (threadIdx.x < 64) exp_tab[threadIdx.x] = ndtm::c_exp2_64[threadIdx.x];
  __syncthreads();                                 // (the only block barrier of the kernel, before the persistent loop)
  // the control block of the NEXT round (k_update fills it after this kernel) is cleared here, not by a host memset
  if (blockIdx.x == 0 && threadIdx.x < 9) reinterpret_cast<int*>(ctl_next)[threadIdx.x] = 0;
  if (FINE && sc.host_flags && blockIdx.x == 0 && threadIdx.x == 0) {     // progress report of the latency-mode pump (posted writes over PCIe)
    sc.host_flags[1] = n_active;
    __threadfence_system();
    sc.host_flags[0] = sc.seq_no;
  }
  if (n_active == 0) return;                       // nothing left to sweep (the loop's last, empty round)
  // Latency mode: the re-basing of p that the NEXT Newton update starts with -- log(exp(delta_p) exp(p)) and float(exp(delta_p)), impl2:163-166 --
  // depends only on what the previous update decided (p, dir, a_t), not on this sweep.  One extra workgroup computes it while the others
  // sweep (two SE(3) exponentials and a logarithm: ~9 k cycles of a serial f64 chain that used to sit on the update's critical path); the
  // update picks it up behind the tag (= the pair's sweep count), exactly as the one-launch align does (ndt_async.hpp).
  const int nblk = FINE && sc.rebase_block ? (int)gridDim.x - 1 : (int)gridDim.x;
  if (FINE && sc.rebase_block && (int)blockIdx.x == nblk) {
    if (wv != 0) return;
    for (int a = 0; a < n_active; a++) {
      PairState& S = const_cast<PairState&>(st[active_list[a]]);
      if (S.phase != PH_STEP) continue;              // (wave-uniform: the first sweep of an align has no step behind it)
      double pn[6]; float inc[16];
      newton_rebase(S.p, S.dir, S.a_t, pn, inc);
      if (lane == 0) {
        for (int k = 0; k < 6; k++) S.reb_pn[k] = pn[k];
        for (int k = 0; k < 16; k++) S.reb_inc[k] = inc[k];
        S.reb_tag = (long long)S.sweeps;
      }
    }
    return;
  }
  const int my_xcd = blockIdx.x & 7;
  // Items of a queue are handed out in two ways.  The first `n_static` rounds are STATIC: wave `wx` of the XCD's `xw` waves takes
  // items wx, wx + xw, ...; only the rest of the queue is claimed with an atomic.  Why: VMEM operations of a wave complete in
  // order (vmcnt), so every load issued after a returning atomic -- an agent-scope atomic takes ~4 us here -- waits for it;
  // with one claim per item the point loads of every item sat behind one (measured with -DNDT_TIMELINE: 10 k cycles per item).
  // The dynamic tail (1 / 2^sc.dyn_shift of the queue, more when that is no whole round) absorbs the imbalance.
  // FLAT dealing: one queue over all active pairs, item i to wave i of the whole grid (then i + all waves, ...), no atomics and no
  // XCD affinity.  Always in latency mode; in batch mode whenever the launch has no more items than waves -- the last rounds of a
  // batch, when a handful of pairs are still iterating: with fewer than eight active pairs most XCDs own no queue and their waves
  // would do nothing but steal, one returning atomic (~4 us) per item.  Which wave runs an item is no part of its result.
  const bool flat = FINE || (n_active * items_per_pair <= nblk * WAVES);
  const int xw = flat ? nblk * WAVES : (int)(gridDim.x >> 3) * WAVES;                    // waves per XCD (flat: of the whole grid)
  const int wx = flat ? (int)blockIdx.x * WAVES + wv : (int)(blockIdx.x >> 3) * WAVES + wv;
  Timeline tl;
#pragma unroll 1
  for (int probe = 0; probe < (flat ? 1 : 8); probe++) {        // own XCD first, then steal (flat: one queue, all static)
    const int xcd = flat ? 0 : (my_xcd + probe) & 7;
    const int pairs_here = flat ? n_active : (n_active > xcd ? (n_active - xcd + 7) / 8 : 0);
    const int items_here = pairs_here * items_per_pair;
    if (items_here == 0) continue;
    // static rounds of this queue (the same number for every wave; none when the grid is no multiple of 8 or for a thief)
    const int n_static = flat ? (items_here + xw - 1) / xw : (((gridDim.x & 7) == 0) ? (items_here - (items_here >> sc.dyn_shift)) / xw : 0);
    const int dyn0 = n_static * xw;               // first item of the dynamic tail
    int round = 0;
    const bool own = flat || ((probe == 0) && n_static > 0);
    int item = 0;
    if (own) item = wx;
    else {
      // a drained queue is recognised with a plain (L2) load; only a queue that still has items costs an atomic
      if (dyn0 + __hip_atomic_load(&ctl->next_item[xcd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= items_here) continue;
      if (lane == 0) item = dyn0 + atomicAdd(&ctl->next_item[xcd], 1);
      item = __builtin_amdgcn_readfirstlane(item);
    }
#pragma unroll 1
    while (item < items_here) {
      // the next item: static while rounds are left, else claimed NOW (the atomic's round trip is hidden behind this item's work)
      const bool next_static = own && (round + 1 < n_static);
      int next_item = 0;
      if (flat) next_item = items_here;             // no dynamic tail
      else if (!next_static && lane == 0) next_item = dyn0 + atomicAdd(&ctl->next_item[xcd], 1);
      const int b = active_list[flat ? item / items_per_pair : xcd + 8 * (item / items_per_pair)];
      const int rem = item % items_per_pair;        // the pair's work item = its partial row
      TL_STAMP(0);

      sweep_item<PCA, K, IT, FINE, ORD, false, false, PM, false, GATE>(b, rem, src, pitch, st, gd, words, recs, partials, rows_per_pair, sc, cent, grid_of, exp_tab, 0u, 0, 0, tl);
      if (next_static) { round++; item = wx + round * xw; }
      else item = __builtin_amdgcn_readfirstlane(next_item);
    }
  }
  tl.flush(0, 8);
}
