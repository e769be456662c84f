// icp_outer.hpp -- the host half of pcl::IterativeClosestPoint::computeTransformation (PCL 1.8, RESTATED AS RECALLED: PCL is not in the
// reference tree; parity unpinned): the rigid estimate of TransformationEstimationSVD (Eigen::umeyama without scaling) from
// the step's sixteen sums, DefaultConvergenceCriteria::hasConverged, and the loop over an evaluator of "one step".  Plain C++: nothing of
// HIP, nothing of the handle (ndtm::jacobi_svd3 comes from ndt_math.hpp).  tools/icp_ref.py restates it.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "mi355_ndt.h"

static const float ICP_IDENTITY[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};

struct IcpSums { double v[16]; int m; };            // sum p [0..2], sum q [3..5], sum q_r p_c [6 + 3 r + c], sum d2 [15]; the matches

// transformation (column-major f32) = [R | t], R = U diag(1, 1, s) V', s = -1 iff det U * det V < 0, t = cq - R cp, over
// Sigma = (sum q p' - (sum q)(sum p)' / m) / m = U S V'
static inline void icp_estimate(const IcpSums& a, float T[16]) {
  const double m = (double)a.m;
  double cp[3], cq[3], Sg[9], U[9], S[3], V[9], R[9];
  for (int r = 0; r < 3; r++) { cp[r] = a.v[r] / m; cq[r] = a.v[3 + r] / m; }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Sg[3 * r + c] = (a.v[6 + 3 * r + c] - a.v[3 + r] * a.v[c] / m) / m;
  ndtm::jacobi_svd3(Sg, U, S, V);
  auto det = [](const double* M) {
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  };
  const double s = det(U) * det(V) < 0.0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + (U[3 * r + 2] * s) * V[3 * c + 2];
  memcpy(T, ICP_IDENTITY, sizeof ICP_IDENTITY);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[c * 4 + r] = (float)R[3 * r + c];
    T[3 * 4 + r] = (float)(cq[r] - ((R[3 * r] * cp[0] + R[3 * r + 1] * cp[1]) + R[3 * r + 2] * cp[2]));
  }
}

// C = A B, column-major f32 4x4, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
static inline void icp_mul4(const float* A, const float* B, float* C) {
  float o[16];
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++) o[c * 4 + r] = ((A[0 * 4 + r] * B[c * 4 + 0] + A[1 * 4 + r] * B[c * 4 + 1]) + A[2 * 4 + r] * B[c * 4 + 2]) + A[3 * 4 + r] * B[c * 4 + 3];
  memcpy(C, o, sizeof o);
}

// one pair's run of computeTransformation between two steps
struct IcpRun {
  float fin[16];                                   // final_transformation_
  float T[16];                                     // what the NEXT step moves the working cloud by (first: the guess, from the source rows)
  bool first = true, ended = false, pending = false;   // pending: T is estimated and the working cloud has not been moved by it yet
  int nr = 0, state = MI355NDT_ICP_NOT_CONVERGED, matches = 0;
  bool converged = false;
  double prev_mse = DBL_MAX, mse = 0.0;
};

static inline void icp_begin(IcpRun& r, const float* guess) {
  r = IcpRun();
  memcpy(r.fin, guess, sizeof r.fin);
  memcpy(r.T, guess, sizeof r.T);
}

// the step's record is in: the estimate and the criteria.  True when the run has ended.
static inline bool icp_advance(IcpRun& r, const mi355ndt_icp_params& p, const IcpSums& a) {
  r.first = false; r.pending = false;
  r.matches = a.m;
  r.mse = a.m > 0 ? a.v[15] / (double)a.m : 0.0;
  if (a.m < p.min_number_correspondences || a.m < 1) {                           // converged_ = false, CONVERGENCE_CRITERIA_NO_CORRESPONDENCES
    r.converged = false; r.state = MI355NDT_ICP_NO_CORRESPONDENCES; r.ended = true;
    return true;
  }
  icp_estimate(a, r.T);
  r.pending = true;                                                              // (the next step, or get_aligned, moves the cloud)
  icp_mul4(r.T, r.fin, r.fin);
  r.nr++;
  // DefaultConvergenceCriteria::hasConverged, in its order
  const float* T = r.T;
  if (r.nr >= p.max_iterations) { r.state = MI355NDT_ICP_ITERATIONS; r.converged = true; }
  else {
    const double cos_angle = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
    const double tr2 = ((double)T[12] * (double)T[12] + (double)T[13] * (double)T[13]) + (double)T[14] * (double)T[14];
    // (the squared translation against the unsquared epsilon: PCL's slip, reproduced)
    if (cos_angle >= 1.0 - p.transformation_epsilon && tr2 <= p.transformation_epsilon) { r.state = MI355NDT_ICP_TRANSFORM; r.converged = true; }
    else if (fabs(r.mse - r.prev_mse) < 1e-12) { r.state = MI355NDT_ICP_ABS_MSE; r.converged = true; }
    else if (fabs(r.mse - r.prev_mse) / r.prev_mse < p.euclidean_fitness_epsilon) { r.state = MI355NDT_ICP_REL_MSE; r.converged = true; }
    else r.prev_mse = r.mse;
  }
  r.ended = r.converged;
  return r.ended;
}

static inline void icp_result(const IcpRun& r, mi355ndt_icp_result* out) {
  memcpy(out->final_colmajor, r.fin, sizeof r.fin);
  out->converged = r.converged ? 1 : 0; out->iterations = r.nr; out->state = r.state; out->matches = r.matches; out->mse = r.mse;
}

// computeTransformation for K pairs against one target over an evaluator of one step for the pairs that have not ended:
//   int step(const int* slots, int n, const IcpRun* runs, IcpSums* sums)   slot k = slots[j]: move by runs[k].T (runs[k].first: from the
//                                                                          source rows), match, sum -> sums[k]; non-zero ends everything
// The single-pair surface (K = 1) and the batch both run this one copy, which is what makes their bytes equal.  rounds / requests: the
// steps of the longest run / of each run.
template <typename Eval>
static int icp_outer(Eval& ev, const mi355ndt_icp_params& p, int K, const float* guesses, std::vector<IcpRun>& runs, int* rounds, int* requests) {
  runs.assign((size_t)K, IcpRun());
  std::vector<IcpSums> sums((size_t)K);
  std::vector<int> active, next;
  for (int k = 0; k < K; k++) { icp_begin(runs[(size_t)k], guesses + 16 * (size_t)k); active.push_back(k); if (requests) requests[k] = 0; }
  int nrounds = 0;
  while (!active.empty()) {
    const int rc = ev.step(active.data(), (int)active.size(), runs.data(), sums.data());
    nrounds++;
    if (rounds) *rounds = nrounds;
    if (rc) return rc;
    next.clear();
    for (int k : active) {
      if (requests) requests[k]++;
      if (!icp_advance(runs[(size_t)k], p, sums[(size_t)k])) next.push_back(k);
    }
    active.swap(next);
  }
  if (rounds) *rounds = nrounds;
  return 0;
}
