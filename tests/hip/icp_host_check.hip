// TEST HELPER: the host-only pieces of the ICP surface -- ndtm::jacobi_svd3 (ndt_math.hpp), the rigid estimate, the convergence criteria and
// icp_outer (icp_outer.hpp) -- over a CPU evaluator of "one step" (exhaustive search, sums in index order), as a stand-alone program for a
// sanitizer run of the host code.  It makes no HIP call and needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude -Ilv_slam_amd/csrc \
//         tests/hip/icp_host_check.hip -o icp_host_check && ./icp_host_check
// Exit status 0 and "icp_host_check: ok" when every check holds.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mi355_ndt.h"
#include "ndt_math.hpp"
#include "icp_outer.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Cloud { std::vector<float> x, y, z; size_t n() const { return x.size(); } };

static unsigned long long rng_state = 88172645463325252ull;
static double uniform() {                            // xorshift64: a fixed sequence
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

static void move(const float* T, float& x, float& y, float& z) {
  const float a = x, b = y, c = z;
  x = ((T[0] * a + T[4] * b) + T[8] * c) + T[12];
  y = ((T[1] * a + T[5] * b) + T[9] * c) + T[13];
  z = ((T[2] * a + T[6] * b) + T[10] * c) + T[14];
}

// the CPU evaluator: every slot has its own working cloud; the target is shared
struct EvalCpu {
  const Cloud& tgt; std::vector<const Cloud*> src; std::vector<Cloud> W; double thr2; int calls = 0, fail_at = -1;
  int step(const int* slots, int n, const IcpRun* runs, IcpSums* sums) {
    if (calls++ == fail_at) return MI355NDT_ERR_HIP;
    for (int j = 0; j < n; j++) {
      const int k = slots[j];
      if (runs[k].first) W[(size_t)k] = *src[(size_t)k];
      Cloud& w = W[(size_t)k];
      IcpSums& o = sums[k];
      memset(&o, 0, sizeof o);
      for (size_t i = 0; i < w.n(); i++) {
        move(runs[k].T, w.x[i], w.y[i], w.z[i]);
        if (!std::isfinite(w.x[i]) || !std::isfinite(w.y[i]) || !std::isfinite(w.z[i])) continue;
        float best = INFINITY; size_t bj = tgt.n();
        for (size_t t = 0; t < tgt.n(); t++) {
          const float dx = w.x[i] - tgt.x[t], dy = w.y[i] - tgt.y[t], dz = w.z[i] - tgt.z[t];
          const float d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2 < best) { best = d2; bj = t; }
        }
        if (bj == tgt.n() || !((double)best <= thr2)) continue;
        const double p[3] = {w.x[i], w.y[i], w.z[i]}, q[3] = {tgt.x[bj], tgt.y[bj], tgt.z[bj]};
        for (int r = 0; r < 3; r++) {
          o.v[r] += p[r]; o.v[3 + r] += q[r];
          for (int c = 0; c < 3; c++) o.v[6 + 3 * r + c] += q[r] * p[c];
        }
        o.v[15] += (double)best;
        o.m++;
      }
    }
    return 0;
  }
};

static void rot_z(double a, double R[9]) { const double c = cos(a), s = sin(a); const double r[9] = {c, -s, 0, s, c, 0, 0, 0, 1}; memcpy(R, r, sizeof r); }

int main() {
  // ---- the SVD: random, rank-deficient and zero matrices
  for (int trial = 0; trial < 3000; trial++) {
    double A[9], U[9], S[3], V[9];
    double a[3], b[3], c[3], d[3];
    for (int i = 0; i < 3; i++) { a[i] = uniform() - 0.5; b[i] = uniform() - 0.5; c[i] = uniform() - 0.5; d[i] = uniform() - 0.5; }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++)
        A[3 * i + j] = trial % 4 == 0 ? uniform() - 0.5 : (trial % 4 == 1 ? a[i] * b[j] : (trial % 4 == 2 ? a[i] * b[j] + c[i] * d[j] : 0.0));
    const double scale = trial % 4 == 3 ? 1.0 : pow(10.0, (double)(trial % 31) - 15.0);
    for (int i = 0; i < 9; i++) A[i] *= scale;
    ndtm::jacobi_svd3(A, U, S, V);
    CHECK(S[0] >= S[1] && S[1] >= S[2] && S[2] >= 0.0);
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double rec = 0.0, uu = 0.0, vv = 0.0;
        for (int k = 0; k < 3; k++) { rec += U[3 * i + k] * S[k] * V[3 * j + k]; uu += U[3 * k + i] * U[3 * k + j]; vv += V[3 * k + i] * V[3 * k + j]; }
        worst = fmax(worst, fabs(rec - A[3 * i + j]) / (S[0] > 0.0 ? S[0] : 1.0));
        worst = fmax(worst, fmax(fabs(uu - (i == j)), fabs(vv - (i == j))));
      }
    CHECK(worst <= 1e-13);
    if (trial % 4 == 3) CHECK(U[0] == 1.0 && U[4] == 1.0 && U[8] == 1.0 && V[0] == 1.0 && S[0] == 0.0);
  }
  // ---- the estimate: a lattice and its copy under a known motion; a mirrored planar cloud (the reflection branch)
  Cloud src, tgt;
  double Rz[9];
  rot_z(0.01, Rz);
  const double t[3] = {0.15, -0.1, 0.05};
  for (int i = 0; i < 5; i++)
    for (int j = 0; j < 5; j++)
      for (int k = 0; k < 5; k++) {
        const double p[3] = {i - 2.0 + 0.2 * (uniform() - 0.5), j - 2.0 + 0.2 * (uniform() - 0.5), k - 2.0 + 0.2 * (uniform() - 0.5)};
        src.x.push_back((float)p[0]); src.y.push_back((float)p[1]); src.z.push_back((float)p[2]);
        const double sp[3] = {(double)src.x.back(), (double)src.y.back(), (double)src.z.back()};
        tgt.x.push_back((float)(Rz[0] * sp[0] + Rz[1] * sp[1] + Rz[2] * sp[2] + t[0]));
        tgt.y.push_back((float)(Rz[3] * sp[0] + Rz[4] * sp[1] + Rz[5] * sp[2] + t[1]));
        tgt.z.push_back((float)(Rz[6] * sp[0] + Rz[7] * sp[1] + Rz[8] * sp[2] + t[2]));
      }
  Cloud one;                                         // a single point: fewer than three correspondences
  one.x.push_back(0.f); one.y.push_back(0.f); one.z.push_back(0.f);
  Cloud nan = src;
  nan.x[3] = NAN; nan.z[17] = INFINITY;
  mi355ndt_icp_params prm = {0.01, 64, -DBL_MAX, sqrt(DBL_MAX), 3, 0};
  float G[3 * 16];
  for (int k = 0; k < 3; k++) memcpy(G + 16 * k, ICP_IDENTITY, sizeof ICP_IDENTITY);
  {
    EvalCpu ev{tgt, {&src, &one, &nan}, std::vector<Cloud>(3), prm.corr_dist_threshold * prm.corr_dist_threshold};
    std::vector<IcpRun> runs;
    int rounds = 0, req[3];
    CHECK(icp_outer(ev, prm, 3, G, runs, &rounds, req) == 0);
    CHECK(runs[0].converged && runs[0].state == MI355NDT_ICP_TRANSFORM && runs[0].nr == 2 && runs[0].matches == 125);
    CHECK(!runs[1].converged && runs[1].state == MI355NDT_ICP_NO_CORRESPONDENCES && runs[1].nr == 0 && !runs[1].pending);
    CHECK(runs[2].converged && runs[2].matches == 123);
    CHECK(rounds == 2 && req[0] == 2 && req[1] == 1 && req[2] == 2);
    const float* F = runs[0].fin;
    CHECK(fabs(F[12] - t[0]) <= 1e-6 && fabs(F[13] - t[1]) <= 1e-6 && fabs(F[14] - t[2]) <= 1e-6 && fabs(F[1] - Rz[3]) <= 1e-6 && fabs(F[0] - Rz[0]) <= 1e-6);
    mi355ndt_icp_result res;
    icp_result(runs[0], &res);
    CHECK(res.iterations == 2 && res.converged == 1 && res.mse >= 0.0);
    // every other exit
    mi355ndt_icp_params p2 = prm;
    p2.max_iterations = 1;
    CHECK(icp_outer(ev, p2, 1, G, runs, &rounds, req) == 0 && runs[0].state == MI355NDT_ICP_ITERATIONS && runs[0].converged && runs[0].nr == 1);
    p2 = prm; p2.transformation_epsilon = 0.0;
    CHECK(icp_outer(ev, p2, 1, G, runs, &rounds, req) == 0 && runs[0].state == MI355NDT_ICP_ABS_MSE && runs[0].nr >= 2);
    p2.euclidean_fitness_epsilon = 0.5; p2.max_iterations = 64;
    CHECK(icp_outer(ev, p2, 1, G, runs, &rounds, req) == 0 && (runs[0].state == MI355NDT_ICP_REL_MSE || runs[0].state == MI355NDT_ICP_ABS_MSE));
    p2 = prm; p2.max_iterations = 0;                 // the loop runs once and ends at the cap
    CHECK(icp_outer(ev, p2, 1, G, runs, &rounds, req) == 0 && runs[0].state == MI355NDT_ICP_ITERATIONS && runs[0].nr == 1);
    ev.fail_at = ev.calls + 1;                       // a failed round: nothing more is asked, the error comes back
    const int before = ev.calls;
    CHECK(icp_outer(ev, prm, 3, G, runs, &rounds, req) == MI355NDT_ERR_HIP && ev.calls == before + 2 && rounds == 2);
  }
  {
    IcpSums a;                                       // a planar cloud mirrored in its plane: det U det V < 0, the estimate is a rotation
    memset(&a, 0, sizeof a);
    for (int i = 0; i < 40; i++) {
      const double p[3] = {4.0 * (uniform() - 0.5), 4.0 * (uniform() - 0.5), 0.0}, q[3] = {p[0], -p[1], 0.0};
      for (int r = 0; r < 3; r++) {
        a.v[r] += p[r]; a.v[3 + r] += q[r];
        for (int c = 0; c < 3; c++) a.v[6 + 3 * r + c] += q[r] * p[c];
      }
      a.m++;
    }
    float T[16];
    icp_estimate(a, T);
    const double det = (double)T[0] * ((double)T[5] * T[10] - (double)T[9] * T[6]) - (double)T[4] * ((double)T[1] * T[10] - (double)T[9] * T[2]) +
                       (double)T[8] * ((double)T[1] * T[6] - (double)T[5] * T[2]);
    CHECK(fabs(det - 1.0) <= 1e-6 && fabs(T[0] - 1.f) <= 1e-6 && fabs(T[5] + 1.f) <= 1e-6 && fabs(T[10] + 1.f) <= 1e-6);
  }
  printf(failures ? "icp_host_check: %d checks failed\n" : "icp_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
