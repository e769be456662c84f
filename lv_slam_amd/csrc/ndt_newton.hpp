// ndt_newton.hpp -- Newton control on the device as plain device functions: computeTransformation's loop body and the live prefix of
// computeStepLengthMT (include/ndt_omp/ndt_omp_impl2.hpp:87-188, 841-907), plus the pose set-up of one pair.  No kernel and no memory
// protocol lives here: the three update routes (ndt_update.hpp, ndt_sequence.hpp, ndt_async.hpp) and the sweep's re-basing workgroup
// (ndt_sweep.hpp) all call these functions, which is what makes their result words the same.
#pragma once
#include "ndt_types.hpp"
#include "ndt_math.hpp"

__device__ void finalize_pair(PairState& S, mi355ndt_result* res, int converged) {
  S.converged = converged;
  S.phase = PH_DONE;
  S.trans_probability = S.score / (double)S.n_src;                                // impl2:149 / 187
  mi355ndt_result o;
  for (int a = 0; a < 16; a++) o.final_colmajor[a] = S.final_cm[a];
  o.trans_probability = S.trans_probability;
  o.score = S.score;
  o.iterations = S.it;
  o.converged = converged;
  o.sweeps = S.sweeps;
  o.status = (S.grid_status == GRID_OK || S.grid_status == GRID_EMPTY) ? MI355NDT_OK : MI355NDT_ERR_GRID;
  o.hits_last = S.hits;
  *res = o;
}

__device__ __forceinline__ double shfl_d(double v, int src) { return __shfl(v, src); }
__device__ __forceinline__ ndtm::SE3 shfl_se3(const ndtm::SE3& e, int src) {
  ndtm::SE3 r;
  r.q.w = shfl_d(e.q.w, src); r.q.x = shfl_d(e.q.x, src); r.q.y = shfl_d(e.q.y, src); r.q.z = shfl_d(e.q.z, src);
  r.t[0] = shfl_d(e.t[0], src); r.t[1] = shfl_d(e.t[1], src); r.t[2] = shfl_d(e.t[2], src);
  return r;
}

// ---- the pose model (MI355NDT_OPT_POSE_MODEL) behind the one update body ------------------------------------------------
// PM = 0: ndt_omp_impl2.hpp -- p is the tangent of SE(3), a step re-bases it (newton_rebase), T = float(exp(p)), Rj = its rotation.
// PM = 1: ndt_omp_impl.hpp  -- p = [x y z roll pitch yaw], a step adds to it (impl.hpp:152), T = convertTransform(p) in f32 (impl.hpp:811-814),
//         transformation_ = convertTransform(delta_p) (impl.hpp:146-149); whoever writes T writes the pair's 23 rows for the sweep that reads it
//         (`rows`: the pair's slot of SweepConst::euler_rows).  Rj, reb_* and the re-basing are not used.
//         `rows64` non-null (MI355NDT_OPT_NDT_CLASS = 1, PCL's f64 class): the rows are written as doubles there (SweepConst::pcl_rows) and
//         `rows` is left alone -- the one difference the class makes on this side of the sweep.
// the pair's rows at pose vector x, in the form its sweep reads
__device__ __forceinline__ void write_pose_rows(const double x[6], float* rows, double* rows64) {
  if (rows64) ndtm::euler_rows64(x, rows64); else ndtm::euler_rows(x, rows);
}
// The sweep pose of a pair from its pose vector
template <int PM>
__device__ __forceinline__ void pose_to_sweep(const double x[6], PairState& S, float* rows, double* rows64 = nullptr) {
  if constexpr (PM == 1) { ndtm::euler_to_f32(x, S.T); write_pose_rows(x, rows, rows64); }
  else ndtm::pose_to_f32(x, S.T, S.Rj);
}
// A step of length a_t along dir taken from p (PM = 1): pn = p + delta_p, inc = convertTransform(delta_p)
__device__ inline void euler_step(const double p[6], const double dir[6], const double a_t, double pn[6], float inc_cm[16]) {
  double dp[6];
  for (int a = 0; a < 6; a++) { dp[a] = dir[a] * a_t; pn[a] = p[a] + dp[a]; }    // impl.hpp:143, 152
  ndtm::euler_to_cm(dp, inc_cm);                                                 // impl.hpp:146-149
}

// computeTransformation's set-up for one pair (impl2:102-129): p = log(guess), first sweep moves the cloud by the f32 guess itself
// PM = 1 (impl.hpp:95-119): p = the f32 translation and f32 rotation().eulerAngles(0, 1, 2) of the guess, widened; the rows from that p
template <int PM = 0>
__device__ inline void init_pair_state(PairState& S, const float G[16] /* column-major */, int n_src, int grid_status, float* rows = nullptr,
                                       double* rows64 = nullptr) {
  double R[9], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) { S.T[r * 4 + c] = G[c * 4 + r]; R[r * 3 + c] = (double)G[c * 4 + r]; }
    S.T[r * 4 + 3] = G[12 + r];
    t[r] = (double)G[12 + r];
  }
  for (int a = 0; a < 16; a++) S.final_cm[a] = G[a];
  if constexpr (PM == 1) {
    float e[3];
    ndtm::euler_angles_012(G, e);
    for (int a = 0; a < 3; a++) { S.p[a] = t[a]; S.p[3 + a] = (double)e[a]; }
    for (int a = 0; a < 9; a++) S.Rj[a] = 0.f;
    write_pose_rows(S.p, rows, rows64);
  } else {
    ndtm::se3_log(ndtm::se3_from_Rt(R, t), S.p);
    float Tdummy[12];
    ndtm::pose_to_f32(S.p, Tdummy, S.Rj);
  }
  S.it = 0; S.phase = PH_SWEEP0; S.converged = 0; S.sweeps = 1; S.a_t = 0; S.hits = 0; S.score = 0; S.mt_loops = 0; S.last_sweep = 0;
  for (int a = 0; a < 16; a++) S.inc_cm[a] = S.prev_inc_cm[a] = (a % 5 == 0) ? 1.f : 0.f;    // align(): transformation_ = previous_ = I
  S.n_src = n_src;
  S.grid_status = grid_status;
  S.reb_tag = -1;
}

// ---- More-Thuente pieces (impl2:717-838), live only when step_size <= eps/2 (impl2:888) -------------------------------
// std::min / std::max as libstdc++ evaluates them: a NaN first argument is returned unchanged
__device__ inline double mt_cmin(double a, double b) { return b < a ? b : a; }
__device__ inline double mt_cmax(double a, double b) { return a < b ? b : a; }

// updateIntervalMT (impl2:717-755); I = {a_l, f_l, g_l, a_u, f_u, g_u}
__device__ inline bool mt_update_interval(double I[6], double a_t, double f_t, double g_t) {
  if (f_t > I[1]) { I[3] = a_t; I[4] = f_t; I[5] = g_t; return false; }
  if (g_t * (I[0] - a_t) > 0) { I[0] = a_t; I[1] = f_t; I[2] = g_t; return false; }
  if (g_t * (I[0] - a_t) < 0) { I[3] = I[0]; I[4] = I[1]; I[5] = I[2]; I[0] = a_t; I[1] = f_t; I[2] = g_t; return false; }
  return true;
}

// trialValueSelectionMT (impl2:758-838)
__device__ inline double mt_trial_value(const double I[6], double a_t, double f_t, double g_t) {
  const double a_l = I[0], f_l = I[1], g_l = I[2], a_u = I[3], f_u = I[4], g_u = I[5];
  if (f_t > f_l) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    return fabs(a_c - a_l) < fabs(a_q - a_l) ? a_c : 0.5 * (a_q + a_c);
  }
  if (g_t * g_l < 0) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    return fabs(a_c - a_t) >= fabs(a_s - a_t) ? a_c : a_s;
  }
  if (fabs(g_t) <= fabs(g_l)) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double a_n = fabs(a_c - a_t) < fabs(a_s - a_t) ? a_c : a_s;
    return a_t > a_l ? mt_cmin(a_t + 0.66 * (a_u - a_t), a_n) : mt_cmax(a_t + 0.66 * (a_u - a_t), a_n);
  }
  const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
  const double w = sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}

// The loop of computeStepLengthMT (impl2:920-994) after the first trial's sweep has been reduced into S.score / S.g.
// With step_max <= step_min every clamped trial value is step_min again (or NaN, which std::min/max let through), so the
// reference re-sweeps an unchanged pose: those evaluations are reused here, not re-run (identical by determinism); a NaN
// trial value means a NaN cloud, which has no neighbours (score, gradient = 0).  Returns step_iterations.
__device__ inline int mt_loop(PairState& S, double step_max, double step_min) {
  const double mu = 1.e-4, nu = 0.9;
  const double phi_0 = S.phi0, d_phi_0 = S.dphi0;
  // auxilaryFunction_PsiMT / dPsiMT (ndt_omp.h:480-496) at a = 0
  double I[6] = {0, phi_0 - phi_0 - mu * d_phi_0 * 0.0, d_phi_0 - mu * d_phi_0, 0, phi_0 - phi_0 - mu * d_phi_0 * 0.0, d_phi_0 - mu * d_phi_0};
  bool interval_converged = (step_max - step_min) > 0, open_interval = true;      // impl2:888
  double a_t = S.a_t;
  const double score_c = S.score;
  double g_c[6];
  for (int a = 0; a < 6; a++) g_c[a] = S.g[a];
  double score = score_c, gd = 0;
  for (int a = 0; a < 6; a++) gd += g_c[a] * S.dir[a];
  double phi_t = -score, d_phi_t = -gd;
  double psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t, d_psi_t = d_phi_t - mu * d_phi_0;
  int its = 0;
  while (!interval_converged && its < 10 && !(psi_t <= 0 && d_phi_t <= -nu * d_phi_0)) {
    a_t = open_interval ? mt_trial_value(I, a_t, psi_t, d_psi_t) : mt_trial_value(I, a_t, phi_t, d_phi_t);
    a_t = mt_cmax(mt_cmin(a_t, step_max), step_min);                             // impl2:936-937
    if (a_t != a_t) { score = 0; gd = 0; } else { score = score_c; gd = 0; for (int a = 0; a < 6; a++) gd += g_c[a] * S.dir[a]; }
    phi_t = -score; d_phi_t = -gd;
    psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t; d_psi_t = d_phi_t - mu * d_phi_0;
    if (open_interval && (psi_t <= 0 && d_psi_t >= 0)) {                         // impl2:963-974
      open_interval = false;
      I[1] = I[1] + phi_0 - mu * d_phi_0 * I[0]; I[2] = I[2] + mu * d_phi_0;
      I[4] = I[4] + phi_0 - mu * d_phi_0 * I[3]; I[5] = I[5] + mu * d_phi_0;
    }
    interval_converged = open_interval ? mt_update_interval(I, a_t, psi_t, d_psi_t) : mt_update_interval(I, a_t, phi_t, d_phi_t);
    its++;
  }
  S.a_t = a_t;
  return its;
}

enum { NEWTON_DONE = 0, NEWTON_SWEEP = 1, NEWTON_HESSIAN = 2 };

// impl2:138-140: JacobiSVD(H).solve(-g).  Well-conditioned H: exact LU solve (same answer to rounding); anything else
// (rank-deficient, H = 0, ill-conditioned): the thresholded pseudo-inverse itself.  (Non-finite g or H: the SVD route answers NaN,
// as Eigen's does, and the pair ends with converged = 0.)
__device__ __forceinline__ void newton_solve(const PairState& S, double d[6]) {
  double neg[6];
  for (int a = 0; a < 6; a++) neg[a] = -S.g[a];
  bool fin = true;
  for (int a = 0; a < 36; a++) fin = fin && isfinite(S.H[a]);
  for (int a = 0; a < 6; a++) fin = fin && isfinite(S.g[a]);
  if (!fin || !ndtm::lu_solve6(S.H, neg, d)) ndtm::svd_solve6(S.H, neg, d);
}
// When the More-Thuente loop is dead (mt = 0) the solve depends only on the reduced (g, H) -- not on the re-basing of p that
// wave 0 runs first -- so a second wave of the block computes it at the same time and hands it over through LDS
// (`sol`: d[6], then a ready flag).  Same function, same inputs: same bits.
//
// (Round 5 also built the elimination ROW-PARALLEL -- lane i < 6 owning row i of the 6 x 13 tableau [H | I | -g], pivot candidates by
// v_readlane, the row permutation by ds_bpermute, back substitution column-parallel through LDS: ~1 k instead of ~3 k instructions, bit-identical
// (tests/test_solve6_gpu.py) -- and measured it slower: 20.6 k against 16 k cycles per update inside the one-launch align, 13.7 k for the solve
// wave of k_seq_update; the cross-lane traffic of a 6-wide problem costs more than the straight-line code it saves.  docs/experiments.md 10d.)
#define SOL_WORDS 8
__device__ __forceinline__ void newton_solve_side(const PairState& S, volatile double* sol) {
  // lanes 0..5 eliminate [H | e_k] (the columns of H^-1, for the condition estimate), lane 6 [H | -g]: the seven eliminations of
  // ndtm::lu_solve6 side by side -- same functions, same operands, same order of the final sum: same bits, same decision
  const int lane = threadIdx.x & 63;
  if (lane > 6) return;
  double rhs[6], x[6];
  for (int a = 0; a < 6; a++) rhs[a] = lane < 6 ? (a == lane ? 1.0 : 0.0) : -S.g[a];
  bool fin = true;
  for (int a = 0; a < 36; a++) fin = fin && isfinite(S.H[a]);
  for (int a = 0; a < 6; a++) fin = fin && isfinite(S.g[a]);
  double pmin, pmax;
  bool ok = fin && ndtm::lu_solve6_rhs(S.H, rhs, x, pmin, pmax);                 // (the pivots depend on H only: `ok` is the same on all seven lanes)
  const double c2 = (ok && lane < 6) ? ndtm::norm2_6(x) : 0.0;                   // column `lane` of H^-1
  const double r2 = lane < 6 ? ndtm::norm2_6(S.H + 6 * lane) : 0.0;              // row `lane` of H
  double hF2 = 0, invF2 = 0;
  for (int k = 0; k < 6; k++) { invF2 += __shfl(c2, k); hF2 += __shfl(r2, k); }
  if (lane != 6) return;
  ok = ok && ndtm::lu_accept(hF2, invF2);
  if (!ok) ndtm::svd_solve6(S.H, rhs, x);
  for (int a = 0; a < 6; a++) sol[a] = x[a];
  __threadfence_block();
  sol[6] = 1.0;
}

// ---- the expressions of one Newton step that more than one route needs, once each --------------------------------------
// transformation_ = (Sophus::SE3::exp(delta_p).matrix()).cast<float>() (impl2:163), column-major; `e` = exp(delta_p)
__device__ inline void increment_cm(const ndtm::SE3& e, float inc_cm[16]) {
  double R[9];
  ndtm::q_to_matrix(e.q, R);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) inc_cm[c * 4 + r] = (float)R[r * 3 + c];
    inc_cm[12 + r] = (float)e.t[r];
    inc_cm[r * 4 + 3] = 0.f;
  }
  inc_cm[15] = 1.f;
}

// The re-basing step of impl2:163-166: pn = log(exp(delta_p) exp(p)), inc = float(exp(delta_p)), delta_p = dir * a_t (impl2:156).
// WAVE: called by every lane of a wave -- the two exponentials run side by side on lanes 0 and 1 (SIMT runs them for the price of one)
// and are exchanged by shuffles; results on lane 0.  Otherwise: one after the other on the calling lane.  Same functions, same operands:
// same bits (tests/test_se3_gpu.py holds the two forms against each other word for word).
template <bool WAVE = true>
__device__ __forceinline__ void newton_rebase(const double p[6], const double dir[6], const double a_t, double pn[6], float inc_cm[16]) {
  ndtm::SE3 e_dp, e_p;
  if (WAVE) {
    const int lane = threadIdx.x & 63;
    double in[6];
    for (int a = 0; a < 6; a++) in[a] = (lane & 1) ? p[a] : dir[a] * a_t;
    const ndtm::SE3 e = ndtm::se3_exp(in);
    e_dp = shfl_se3(e, 0);
    e_p = shfl_se3(e, 1);
  } else {
    double dp[6];
    for (int a = 0; a < 6; a++) dp[a] = dir[a] * a_t;
    e_dp = ndtm::se3_exp(dp);
    e_p = ndtm::se3_exp(p);
  }
  increment_cm(e_dp, inc_cm);
  ndtm::se3_log(ndtm::se3_mul(e_dp, e_p), pn);
}

// getFinalTransformation() while the pair runs: the f32 sweep pose, column-major
__device__ inline void pose_to_final(PairState& S) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 4; c++) S.final_cm[c * 4 + r] = S.T[r * 4 + c];
    S.final_cm[r * 4 + 3] = 0.f;
  }
  S.final_cm[15] = 1.f;
}

// impl2:175-179: the step of length a_t taken at iteration count `it` ends the pair.  Reads the count and the step length alone, never
// the sweep's sums: it is decided as soon as the step is scheduled (PairState::last_sweep).
// ground (MI355NDT_OPT_GROUND_CLASS != 0): ndt_ground_impl.hpp:173 has no `nr_iterations_ &&` in front of the step test, so the first step can end the pair.
__device__ inline bool step_ends_pair(const int it, const double a_t, const double eps, const int max_iterations, const bool ground = false) {
  return (it > max_iterations) || ((ground || it) && (fabs(a_t) < eps));
}

// The body of the while loop of computeTransformation (impl2:131-183) with computeStepLengthMT (impl2:841-1003), for one pair
// whose reduced (score, g, H) are in S.  Called by every lane of one wave; lane 0 carries the state, the others only help with the
// re-basing (newton_rebase).  Returns on lane 0: NEWTON_DONE (pair finalised), NEWTON_SWEEP (a step was scheduled: the pair takes part
// in the next derivative sweep), NEWTON_HESSIAN (live More-Thuente case: waiting for the computeHessian pass).
// mt = 0: step_size > eps/2, the More-Thuente loop is dead (every shipped configuration);
// mt = 1: live case, called after a derivative sweep;  mt = 2: live case, called after the computeHessian pass.
// score_only_last (one-launch align, MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP): mark a scheduled step whose convergence test is decided already
// (S.last_sweep), so that its sweep evaluates the score alone.
// PM: the pose model (above); PM = 1 is served with mt = 0 alone, and `rows` is the pair's slot of the Euler rows.
template <int PM = 0>
__device__ __forceinline__ int newton_update(PairState& S, mi355ndt_result* res, double step_max, double eps, int max_iterations, int mt,
                                             volatile double* sol = nullptr /* non-null: the solve comes from newton_solve_side */,
                                             const bool rebased = false /* S.reb_pn / S.reb_inc hold the re-basing of this step already */,
                                             const bool score_only_last = false, float* rows = nullptr, double* rows64 = nullptr,
                                             const int ground = 0 /* MI355NDT_OPT_GROUND_CLASS: the convergence rule above; S holds the doubled, masked sums already */) {
  double pn[6];
  float inc[16];
  const bool pre = PM == 0 && (mt == 0) && (S.phase == PH_STEP) && !rebased;     // wave-uniform: nothing has been written yet
  if (pre) newton_rebase(S.p, S.dir, S.a_t, pn, inc);
  if ((threadIdx.x & 63) != 0) return NEWTON_DONE;

  const double step_min = eps / 2;
  if (mt == 1 && S.phase == PH_STEP) {                                           // impl2:920-1000
    const int its = mt_loop(S, step_max, step_min);
    S.mt_loops += its;
    S.sweeps += its;                                                             // computeDerivatives calls the reference makes
    if (its) {
      bool fin = S.a_t == S.a_t;
      if (!fin) {                                                                // NaN trial value: NaN pose, nothing is hit
        for (int a = 0; a < 6; a++) S.xt[a] = S.p[a] + S.dir[a] * S.a_t;
        ndtm::pose_to_f32(S.xt, S.T, S.Rj);
        pose_to_final(S);
        S.score = 0; S.hits = 0;
        for (int a = 0; a < 6; a++) S.g[a] = 0;
        for (int a = 0; a < 36; a++) S.H[a] = 0;                                 // computeHessian over a NaN cloud
      } else {
        S.phase = PH_HESS;                                                       // impl2:999-1000: H comes from computeHessian
        return NEWTON_HESSIAN;
      }
    }
  }
  if (S.phase == PH_HESS) S.phase = PH_STEP;
  if (S.phase == PH_STEP) {
    if constexpr (PM == 1) {
      euler_step(S.p, S.dir, S.a_t, pn, inc);
    } else if (rebased) {                                                        // computed after the previous update published its sweep (same operations)
      for (int a = 0; a < 16; a++) inc[a] = S.reb_inc[a];
      for (int a = 0; a < 6; a++) pn[a] = S.reb_pn[a];
    } else if (!pre) {                                                           // live More-Thuente: this lane alone
      newton_rebase<false>(S.p, S.dir, S.a_t, pn, inc);
    }
    for (int a = 0; a < 16; a++) S.inc_cm[a] = inc[a];                           // impl2:163
    for (int a = 0; a < 6; a++) S.p[a] = pn[a];                                  // impl2:166
    const bool conv = step_ends_pair(S.it, S.a_t, eps, max_iterations, ground != 0);
#ifdef NDT_DEBUG_LAST_SWEEP
    if (S.last_sweep && !conv) printf("newton_update: last_sweep set for a step that does not end the pair (it %d, a_t %g)\n", S.it, S.a_t);
#endif
    S.it++;
    if (conv) { finalize_pair(S, res, 1); return NEWTON_DONE; }
  }
  for (int guard = 0; guard < 4; guard++) {
    for (int a = 0; a < 16; a++) S.prev_inc_cm[a] = S.inc_cm[a];                 // impl2:134
    double d[6];
    if (sol) {                                                                   // impl2:138-140, computed by the block's second wave meanwhile
      while (sol[6] == 0.0) __builtin_amdgcn_s_sleep(1);
      __threadfence_block();
      for (int a = 0; a < 6; a++) d[a] = sol[a];
    } else {
      newton_solve(S, d);
    }
    double nrm = 0;
    for (int a = 0; a < 6; a++) nrm += d[a] * d[a];
    nrm = sqrt(nrm);
    if (nrm == 0 || nrm != nrm) { finalize_pair(S, res, nrm == nrm); return NEWTON_DONE; }   // impl2:147-152
    for (int a = 0; a < 6; a++) d[a] /= nrm;                                     // impl2:154
    double dphi0 = 0;
    for (int a = 0; a < 6; a++) dphi0 += S.g[a] * d[a];
    dphi0 = -dphi0;                                                              // impl2:849
    if (dphi0 >= 0 && dphi0 == 0) {
      // impl2:856-857: step length 0, nothing re-evaluated
      const double z[6] = {0, 0, 0, 0, 0, 0};
      if constexpr (PM == 1) euler_step(S.p, z, 0.0, pn, S.inc_cm);              // impl.hpp:771-772
      else newton_rebase<false>(S.p, z, 0.0, pn, S.inc_cm);
      for (int a = 0; a < 6; a++) S.p[a] = pn[a];
      const bool conv = step_ends_pair(S.it, 0.0, eps, max_iterations, ground != 0);
      S.it++;
      if (conv) { finalize_pair(S, res, 1); return NEWTON_DONE; }
      continue;
    }
    if (dphi0 >= 0) { for (int a = 0; a < 6; a++) d[a] = -d[a]; }                // impl2:861-862
    double a_t = nrm;
    a_t = a_t < step_max ? a_t : step_max;                                       // impl2:890-892
    a_t = a_t > step_min ? a_t : step_min;
    double xt[6];
    for (int a = 0; a < 6; a++) { S.dir[a] = d[a]; xt[a] = S.p[a] + d[a] * a_t; S.xt[a] = xt[a]; }   // impl2:894
    S.a_t = a_t;
    // the test that follows this step's sweep (above), on the same operands: S.it and a_t are final here.  With the More-Thuente loop
    // live (mt != 0) the sweep's gradient feeds that loop, so it is never marked.
    S.last_sweep = (mt == 0 && score_only_last && step_ends_pair(S.it, a_t, eps, max_iterations, ground != 0)) ? 1 : 0;
    S.phi0 = -S.score;                                                           // impl2:846
    S.dphi0 = dphi0 >= 0 ? -dphi0 : dphi0;                                       // impl2:849, 860
    pose_to_sweep<PM>(xt, S, rows, rows64);                                              // impl2:900 / impl.hpp:811-821
    pose_to_final(S);
    S.phase = PH_STEP;
    S.sweeps++;
    return NEWTON_SWEEP;
  }
  finalize_pair(S, res, 1);
  return NEWTON_DONE;
}
