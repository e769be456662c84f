// TEST HELPER (tests/test_se3_gpu.py): runs the SE(3) half of the Newton control's pose math (ndt_math.hpp: Sophus a621ff2 / Eigen 3.3 restated)
// and the two places of ndt_update.hpp that use it (init_pair_state, newton_rebase) on the device, record by record.  <in.f64> holds records of
// REC_IN doubles, [0] = kind; <out.f64> gets REC_OUT doubles per record.  One wave per record (newton_rebase wants a full wave); everything else
// runs on lane 0.  Flags are 1.0 / 0.0; f32 results are widened to f64 (exact).  The comparison happens in the test.
//   kind 0  in: m[9] q2[4] v[3] t1[3] t2[3]
//           out: q_from_matrix(m)[4: w x y z] | branch (0: trace > 0, 1 + i: trace <= 0, largest diagonal entry i) | qn = q_normalized(.)[4] |
//                q_to_matrix(qn)[9] | q2n = q_normalized(q2)[4] | q_mul(qn, q2n)[4] | q_rotate(qn, v)[3] | se3_mul({qn,t1},{q2n,t2}) q[4] t[3] | mat3_inverse(m)[9]
//   kind 1  in: p[6]          out: se3_exp(p) q[4] t[3] | theta < eps | q_to_matrix(q)[9] | pose_to_f32(p) T[12] Rj[9]
//   kind 2  in: R[9] t[3]     out: se3_log(se3_from_Rt(R, t))[6] | q_from_matrix branch | n < eps | theta < eps (signed) | theta
//   kind 3  in: G[16] (f32 values, column-major)   out: init_pair_state: S.p[6] S.T[12] S.Rj[9] | q_from_matrix branch | theta < eps | theta
//   kind 4  in: p[6] dir[6] a_t
//           out: newton_rebase on a full wave, lane 0: pn[6] inc_cm[16] | the same on one lane alone: se3_log(se3_mul(se3_exp(dir a_t), se3_exp(p)))[6] |
//                w of the product's quaternion | theta < eps | theta
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fhip-fp32-correctly-rounded-divide-sqrt -Ilv_slam_amd/csrc -Iinclude
//          tests/hip/se3_check.hip -o tests/hip/se3_check
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ndt_types.hpp"
#include "ndt_math.hpp"
#include "ndt_newton.hpp"

#define REC_IN 32
#define REC_OUT 72

// The comparisons of ndtm::q_from_matrix restated on the same operands (the library function does not report them): a label for the test's
// bookkeeping.  What holds the library's branch is its result, compared word for word (kind 0).
__device__ inline double q_branch(const double m[9]) {
  if (m[0] + m[4] + m[8] > 0) return 0.0;
  int i = 0;
  if (m[4] > m[0]) i = 1;
  if (m[8] > m[i * 3 + i]) i = 2;
  return 1.0 + i;
}
__device__ inline void put_q(double* o, const ndtm::Quat& q) { o[0] = q.w; o[1] = q.x; o[2] = q.y; o[3] = q.z; }

__global__ void __launch_bounds__(64) k_se3(const double* __restrict__ in, double* __restrict__ out, PairState* st, int n) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const double* r = in + (size_t)i * REC_IN;
  double* o = out + (size_t)i * REC_OUT;
  const int kind = (int)r[0];                                                     // block-uniform
  const int lane = threadIdx.x & 63;
  if (kind == 4) {
    double p[6], dir[6], pn[6];
    float inc[16];
    for (int a = 0; a < 6; a++) { p[a] = r[1 + a]; dir[a] = r[7 + a]; }
    const double a_t = r[13];
    newton_rebase(p, dir, a_t, pn, inc);                                          // every lane of the wave
    if (lane != 0) return;
    for (int a = 0; a < 6; a++) o[a] = pn[a];
    for (int a = 0; a < 16; a++) o[6 + a] = (double)inc[a];
    double dp[6], p1[6];
    for (int a = 0; a < 6; a++) dp[a] = dir[a] * a_t;
    const ndtm::SE3 prod = ndtm::se3_mul(ndtm::se3_exp(dp), ndtm::se3_exp(p));
    ndtm::se3_log(prod, p1);
    for (int a = 0; a < 6; a++) o[22 + a] = p1[a];
    double om[3], theta;
    ndtm::so3_log(prod.q, om, &theta);
    o[28] = prod.q.w; o[29] = theta < NDT_SMALL_EPS ? 1.0 : 0.0; o[30] = theta;
    return;
  }
  if (lane != 0) return;
  if (kind == 0) {
    const double *m = r + 1, *v = r + 14;
    const ndtm::Quat qf = ndtm::q_from_matrix(m);
    put_q(o, qf);
    o[4] = q_branch(m);
    const ndtm::Quat qn = ndtm::q_normalized(qf);
    put_q(o + 5, qn);
    ndtm::q_to_matrix(qn, o + 9);
    const ndtm::Quat q2 = {r[10], r[11], r[12], r[13]};
    const ndtm::Quat q2n = ndtm::q_normalized(q2);
    put_q(o + 18, q2n);
    put_q(o + 22, ndtm::q_mul(qn, q2n));
    ndtm::q_rotate(qn, v, o + 26);
    ndtm::SE3 A, B;
    A.q = qn; B.q = q2n;
    for (int a = 0; a < 3; a++) { A.t[a] = r[17 + a]; B.t[a] = r[20 + a]; }
    const ndtm::SE3 C = ndtm::se3_mul(A, B);
    put_q(o + 29, C.q);
    for (int a = 0; a < 3; a++) o[33 + a] = C.t[a];
    ndtm::mat3_inverse(m, o + 36);
  } else if (kind == 1) {
    double p[6];
    for (int a = 0; a < 6; a++) p[a] = r[1 + a];
    const ndtm::SE3 e = ndtm::se3_exp(p);
    put_q(o, e.q);
    for (int a = 0; a < 3; a++) o[4 + a] = e.t[a];
    double theta;
    ndtm::so3_exp(p + 3, &theta);
    o[7] = theta < NDT_SMALL_EPS ? 1.0 : 0.0;
    ndtm::q_to_matrix(e.q, o + 8);
    float T[12], Rj[9];
    ndtm::pose_to_f32(p, T, Rj);
    for (int a = 0; a < 12; a++) o[17 + a] = (double)T[a];
    for (int a = 0; a < 9; a++) o[29 + a] = (double)Rj[a];
  } else if (kind == 2) {
    const double *R = r + 1, *t = r + 10;
    const ndtm::SE3 s = ndtm::se3_from_Rt(R, t);
    double p[6], om[3], theta;
    ndtm::se3_log(s, p);
    for (int a = 0; a < 6; a++) o[a] = p[a];
    o[6] = q_branch(R);
    ndtm::so3_log(s.q, om, &theta);
    o[7] = sqrt((s.q.x * s.q.x + s.q.y * s.q.y) + s.q.z * s.q.z) < NDT_SMALL_EPS ? 1.0 : 0.0;
    o[8] = theta < NDT_SMALL_EPS ? 1.0 : 0.0;
    o[9] = theta;
  } else if (kind == 3) {
    float G[16];
    for (int a = 0; a < 16; a++) G[a] = (float)r[1 + a];
    PairState& S = st[i];
    init_pair_state(S, G, 1, 0);
    for (int a = 0; a < 6; a++) o[a] = S.p[a];
    for (int a = 0; a < 12; a++) o[6 + a] = (double)S.T[a];
    for (int a = 0; a < 9; a++) o[18 + a] = (double)S.Rj[a];
    double R[9], t[3] = {0, 0, 0}, om[3], theta;
    for (int rr = 0; rr < 3; rr++) for (int c = 0; c < 3; c++) R[rr * 3 + c] = (double)G[c * 4 + rr];
    o[27] = q_branch(R);
    ndtm::so3_log(ndtm::se3_from_Rt(R, t).q, om, &theta);
    o[28] = theta < NDT_SMALL_EPS ? 1.0 : 0.0;
    o[29] = theta;
  }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 3; } } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f) / (REC_IN * sizeof(double));
  fseek(f, 0, SEEK_SET);
  if (n == 0 || n > 65536) { fprintf(stderr, "%zu records\n", n); return 2; }
  std::vector<double> a(n * REC_IN), o(n * REC_OUT, 0.0);
  if (fread(a.data(), sizeof(double), n * REC_IN, f) != n * REC_IN) return 2;
  fclose(f);
  for (size_t i = 0; i < n; i++) {
    const double k = a[i * REC_IN];
    if (!(k == 0 || k == 1 || k == 2 || k == 3 || k == 4)) { fprintf(stderr, "record %zu: kind %g\n", i, k); return 2; }
  }
  double *da = nullptr, *dout = nullptr;
  PairState* st = nullptr;
  CK(hipMalloc((void**)&da, a.size() * sizeof(double)));
  CK(hipMalloc((void**)&dout, o.size() * sizeof(double)));
  CK(hipMalloc((void**)&st, n * sizeof(PairState)));
  CK(hipMemset(st, 0, n * sizeof(PairState)));
  CK(hipMemset(dout, 0, o.size() * sizeof(double)));
  CK(hipMemcpy(da, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice));
  k_se3<<<(unsigned)n, 64>>>(da, dout, st, (int)n);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(o.data(), dout, o.size() * sizeof(double), hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  const bool wrote = fwrite(o.data(), sizeof(double), o.size(), f) == o.size();
  if (fclose(f) != 0 || !wrote) { perror(argv[2]); return 2; }
  CK(hipFree(da));
  CK(hipFree(dout));
  CK(hipFree(st));
  return 0;
}
