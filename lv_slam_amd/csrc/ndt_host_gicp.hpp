// ndt_host_gicp.hpp -- mi355ndt_gicp_*: pclomp::GeneralizedIterativeClosestPoint for one pair, synchronously (kernels: ndt_gicp.hpp; the
// optimiser: gicp_bfgs.hpp).  The host holds what the reference's object holds between calls -- the parameters, the two clouds, their
// covariances -- runs the outer loop of computeTransformation (gicp_omp_impl.hpp:380-515) and the BFGS driver of
// estimateRigidTransformationBFGS (:189-252), and reads one mapped record per evaluation of the cost.  A cloud's index (CloudIndex: a
// keyframe's is the one the fitness scores search, built here if they have not built it) and covariances (GicpCache) are made on first use;
// the index build's sort uses the shared scratch (h->vs).  The batch, the grids, the keyframes' rows, the prefilter result and the other
// workspaces are left as they were.  The pieces the batch form shares (ndt_host_gicp_batch.hpp): GicpSide / GicpView / gicp_prepare, what a
// request takes to the device (gicp_make_match, gicp_make_cost), fdf from the sums (gicp_fdf_sums), the outer loop (gicp_outer).
#pragma once

int mi355ndt_gicp_params_default(mi355ndt_gicp_params* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  p->k_correspondences = 20; p->gicp_epsilon = 1e-3; p->rotation_epsilon = 2e-3;   // gicp_omp.h:110-120
  p->transformation_epsilon = 5e-4; p->max_iterations = 200; p->max_inner_iterations = 20; p->corr_dist_threshold = 5.0;
  return MI355NDT_OK;
}

int mi355ndt_gicp_set_params(mi355ndt_handle* h, const mi355ndt_gicp_params* p) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!p) return MI355NDT_ERR_BAD_ARG;
  if (p->k_correspondences < 1 || p->k_correspondences > OL_MAX_K) { h->err = "gicp_set_params: k_correspondences outside 1..64"; return MI355NDT_ERR_BAD_ARG; }
  if (!(p->gicp_epsilon >= 0) || !(p->rotation_epsilon >= 0) || !(p->transformation_epsilon >= 0) || !(p->corr_dist_threshold >= 0)) {
    h->err = "gicp_set_params: an epsilon or the correspondence distance is NaN or negative"; return MI355NDT_ERR_BAD_ARG;
  }
  if (p->max_iterations < 0 || p->max_inner_iterations < 0) { h->err = "gicp_set_params: a negative iteration count"; return MI355NDT_ERR_BAD_ARG; }
  h->gicp.prm = *p;                               // (the covariances are keyed by k and epsilon: a change is seen at their next use)
  h->gicp.have_corr = false;
  return MI355NDT_OK;
}

// ---- the two clouds -----------------------------------------------------------------------------------
// a host cloud becomes a side's own rows (the single-pair surface's two sides, the batch's slots)
static int gicp_side_set_host(mi355ndt_handle* h, GicpSide& sd, const void* pts, size_t n, size_t stride) {
  if ((n && (!pts || stride < 12)) || n >= (1u << 30)) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));     // nothing enqueued may still read the rows this replaces
  sd.set = false; sd.kf_id = -1;
  sd.n = n; sd.pitch = (n + 63) & ~(size_t)63;
  sd.index.status = CloudIndex::NO_INDEX; sd.cache.k = -1;
  if (sd.pitch) {
    HIPCHK(h, sd.rows_own.reserve(3 * sd.pitch));
    std::vector<float> rows(3 * sd.pitch, 0.f);
    const unsigned char* b = (const unsigned char*)pts;
    for (size_t i = 0; i < n; i++) {
      float v[3];
      memcpy(v, b + i * stride, 12);
      rows[i] = v[0]; rows[sd.pitch + i] = v[1]; rows[2 * sd.pitch + i] = v[2];
    }
    HIPCHK(h, hipMemcpyAsync(sd.rows_own, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  sd.set = true;
  return MI355NDT_OK;
}
static int gicp_set_host(mi355ndt_handle* h, int role, const void* pts, size_t n, size_t stride) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  const int rc = gicp_side_set_host(h, h->gicp.side[role], pts, n, stride);
  if (rc != MI355NDT_ERR_BAD_ARG) h->gicp.have_corr = false;   // (refused arguments change nothing)
  return rc;
}
static int gicp_set_keyframe(mi355ndt_handle* h, int role, int id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!kf_find(h, id, role == MI355NDT_GICP_TARGET ? "gicp_set_target_keyframe" : "gicp_set_source_keyframe")) return MI355NDT_ERR_BAD_ARG;
  GicpSide& sd = h->gicp.side[role];
  sd.kf_id = id; sd.set = true;
  h->gicp.have_corr = false;
  return MI355NDT_OK;
}
int mi355ndt_gicp_set_target(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes) { return gicp_set_host(h, MI355NDT_GICP_TARGET, pts, n, stride_bytes); }
int mi355ndt_gicp_set_source(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes) { return gicp_set_host(h, MI355NDT_GICP_SOURCE, pts, n, stride_bytes); }
int mi355ndt_gicp_set_target_keyframe(mi355ndt_handle* h, int id) { return gicp_set_keyframe(h, MI355NDT_GICP_TARGET, id); }
int mi355ndt_gicp_set_source_keyframe(mi355ndt_handle* h, int id) { return gicp_set_keyframe(h, MI355NDT_GICP_SOURCE, id); }

// a side as the host takes it: the rows, the index and the cache, the surface's own or the keyframe's
struct GicpView { const float* rows; size_t n, pitch; CloudIndex* index; GicpCache* cache; };
static int gicp_view_side(mi355ndt_handle* h, GicpSide& sd, const char* where, const char* unset, GicpView* v) {
  if (!sd.set) { h->err = std::string(where) + unset; return MI355NDT_ERR_STATE; }
  if (sd.kf_id < 0) { *v = GicpView{sd.rows_own, sd.n, sd.pitch, &sd.index, &sd.cache}; return MI355NDT_OK; }
  mi355ndt_handle::Keyframe* kf = kf_find(h, sd.kf_id, where);
  if (!kf) return MI355NDT_ERR_BAD_ARG;
  *v = GicpView{kf->rows, kf->n, kf->pitch, &kf->index, &kf->gicp};
  return MI355NDT_OK;
}
static int gicp_view(mi355ndt_handle* h, int role, const char* where, GicpView* v) {
  return gicp_view_side(h, h->gicp.side[role], where, role == MI355NDT_GICP_TARGET ? ": no target cloud is set" : ": no source cloud is set", v);
}

// the side's index, built at the first use of the cloud (the ICP surface stops here: ndt_host_icp.hpp); waits for the device
static int gicp_prepare_index(mi355ndt_handle* h, const GicpView& v) {
  CloudIndex& ix = *v.index;
  GicpCache& c = *v.cache;
  hipStream_t s = h->stream;
  if (ix.status == CloudIndex::NO_INDEX) {
    int rc = uploads_before_compute(h);           // (a keyframe_add's transfer may still be on its way)
    if (rc) return rc;
    VsNeed need;
    need.pitch = v.pitch; need.stat = 2;
    rc = vs_reserve(h, need);
    if (rc) return rc;
    VoxelScratch& w = h->vs;
    c.k = -1;
    rc = kfi_build_rows(h, v.rows, v.pitch, v.n, h->kff_cell_mm, ix, 0);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(w.h_ret, w.stat, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    w.pending = false;
    HIPCHK(h, hipGetLastError());
    kfi_built(ix, w.h_ret, 0);
  }
  return MI355NDT_OK;
}

// the side's index and its covariances for the current (k_correspondences, gicp_epsilon); waits for the device
static int gicp_prepare(mi355ndt_handle* h, const char* where, const GicpView& v) {
  CloudIndex& ix = *v.index;
  GicpCache& c = *v.cache;
  const int K = h->gicp.prm.k_correspondences;
  const double eps = h->gicp.prm.gicp_epsilon;
  hipStream_t s = h->stream;
  if (v.n == 0) { h->err = std::string(where) + ": k_correspondences exceeds the cloud's searchable points (an empty cloud)"; return MI355NDT_ERR_BAD_ARG; }
  {
    const int rc = gicp_prepare_index(h, v);
    if (rc) return rc;
  }
  if (c.k != K || c.eps != eps) {
    if (K > ix.n_fin) {
      h->err = std::string(where) + ": k_correspondences (" + std::to_string(K) + ") exceeds the cloud's searchable points (" + std::to_string(ix.n_fin) + ")";
      return MI355NDT_ERR_BAD_ARG;
    }
    c.k = -1;
    HIPCHK(h, c.cov.reserve(9 * v.pitch));
    HIPCHK(h, hipMemsetAsync(c.cov, 0, 9 * v.pitch * sizeof(double), s));
    const KfiView view = kfi_view(ix, v.rows, v.pitch, v.n);
    const unsigned blocks = (unsigned)((v.n + OL_LANES - 1) / OL_LANES);
    if (K <= 32) k_gc_cov<32><<<blocks, OL_LANES, 0, s>>>(view, K, eps, c.cov); else k_gc_cov<64><<<blocks, OL_LANES, 0, s>>>(view, K, eps, c.cov);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    c.k = K; c.eps = eps;
  }
  return MI355NDT_OK;
}

// [9][pitch] on the device -> n records of nine f64
static int gicp_fetch9(mi355ndt_handle* h, const double* d, size_t pitch, size_t n, double* out) {
  std::vector<double> tmp(9 * pitch);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), d, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; i++)
    for (int e = 0; e < 9; e++) out[9 * i + e] = tmp[(size_t)e * pitch + i];
  return MI355NDT_OK;
}

int mi355ndt_gicp_covariances(mi355ndt_handle* h, int role, double* out, size_t capacity) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (role != MI355NDT_GICP_TARGET && role != MI355NDT_GICP_SOURCE) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  GicpView v;
  int rc = gicp_view(h, role, "gicp_covariances", &v);
  if (rc) return rc;
  rc = gicp_prepare(h, "gicp_covariances", v);
  if (rc) return rc;
  if (!out) return MI355NDT_OK;
  if (v.n > capacity) { h->err = "gicp_covariances: the cloud has more points than the capacity"; return MI355NDT_ERR_BAD_ARG; }
  return gicp_fetch9(h, v.cache->cov, v.pitch, v.n, out);
}

// ---- f32 pose arithmetic of the host (column-major 4x4) --------------------------------------------------
static const float GICP_IDENTITY[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
// applyState (:517-528): R = AngleAxisf(x5, Z) * AngleAxisf(x4, Y) * AngleAxisf(x3, X) -- Eigen multiplies angle-axes as quaternions
// (w = cos(angle / 2), the axis * sin(angle / 2)) and converts the product to a matrix -- in front of t's rotation; the translation is added
static void gicp_apply_state(float t[16], const double x[6]) {
  struct Q { float w, x, y, z; };
  auto aa = [](double angle, int axis) {
    const float ha = 0.5f * (float)angle;
    const float s = std::sin(ha);
    Q q = {std::cos(ha), 0.f, 0.f, 0.f};
    (axis == 0 ? q.x : axis == 1 ? q.y : q.z) = s;
    return q;
  };
  auto mul = [](Q a, Q b) {
    Q r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
  };
  const Q q = mul(mul(aa(x[5], 2), aa(x[4], 1)), aa(x[3], 0));
  const float tx = 2.f * q.x, ty = 2.f * q.y, tz = 2.f * q.z;
  const float twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const float txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const float tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  const float R[9] = {1.f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.f - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.f - (txx + tyy)};
  float o[16];
  memcpy(o, t, sizeof o);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) o[c * 4 + r] = (R[3 * r] * t[c * 4 + 0] + R[3 * r + 1] * t[c * 4 + 1]) + R[3 * r + 2] * t[c * 4 + 2];
    o[3 * 4 + r] = t[3 * 4 + r] + (float)x[r];
  }
  memcpy(t, o, sizeof o);
}

// ---- correspondences ----------------------------------------------------------------------------------
// what a matching pass with transformation_ = T takes to the device (host arithmetic only)
static GcMatch gicp_make_match(const mi355ndt_gicp_params& p, const float* G, const float* T) {
  GcMatch a;
  memcpy(a.G, G, sizeof a.G); memcpy(a.T, T, sizeof a.T);
  for (int i = 0; i < 3; i++)                     // transform_R (:423-429): f64 products of the f32 entries, k ascending
    for (int j = 0; j < 3; j++) {
      double r = 0.0;
      for (int k = 0; k < 4; k++) r += (double)T[k * 4 + i] * (double)G[j * 4 + k];
      a.R[3 * i + j] = r;
    }
  a.thr2 = p.corr_dist_threshold * p.corr_dist_threshold;
  a.range = (float)a.thr2 * 1.0001f + 1e-30f;     // (f32, above thr2: what lies further cannot match)
  return a;
}
// ... and a cost evaluation at applyState(base, x)
static GcCost gicp_make_cost(const double x[6], const float* base) {
  GcCost a;
  memcpy(a.Tx, base, 16 * sizeof(float)); memcpy(a.B, base, 16 * sizeof(float));
  gicp_apply_state(a.Tx, x);
  return a;
}
// one pass of the matching loop with transformation_ = T; the result stays resident (idx, maha, n_matched)
static int gicp_match(mi355ndt_handle* h, const char* where, const float* G, const float* T) {
  auto& gc = h->gicp;
  gc.have_corr = false;
  GicpView S, D;
  int rc = gicp_view(h, MI355NDT_GICP_TARGET, where, &D);
  if (!rc) rc = gicp_view(h, MI355NDT_GICP_SOURCE, where, &S);
  if (!rc) rc = gicp_prepare(h, where, D);
  if (!rc) rc = gicp_prepare(h, where, S);
  if (rc) return rc;
  hipStream_t s = h->stream;
  HIPCHK(h, gc.idx.reserve(S.pitch)); HIPCHK(h, gc.maha.reserve(9 * S.pitch)); HIPCHK(h, gc.m.reserve(1));
  const GcMatch a = gicp_make_match(gc.prm, G, T);
  HIPCHK(h, hipMemsetAsync(gc.m, 0, sizeof(int), s));
  k_gc_match<<<(unsigned)((S.n + 255) / 256), 256, 0, s>>>(S.rows, S.pitch, (int)S.n, kfi_view(*D.index, D.rows, D.pitch, D.n), a,
                                                           S.cache->cov, D.cache->cov, gc.idx, gc.maha, gc.m);
  HIPCHK(h, hipGetLastError());
  int m = 0;
  HIPCHK(h, hipMemcpyAsync(&m, gc.m, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  gc.n_matched = m;
  gc.have_corr = true;
  return MI355NDT_OK;
}

int mi355ndt_gicp_correspondences(mi355ndt_handle* h, const float* guess_colmajor, const float* T_colmajor, int* idx, double* maha, int* m) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!guess_colmajor) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = gicp_match(h, "gicp_correspondences", guess_colmajor, T_colmajor ? T_colmajor : GICP_IDENTITY);
  if (rc) return rc;
  GicpView S;
  rc = gicp_view(h, MI355NDT_GICP_SOURCE, "gicp_correspondences", &S);
  if (rc) return rc;
  if (m) *m = h->gicp.n_matched;
  if (idx) {
    HIPCHK(h, hipMemcpyAsync(idx, h->gicp.idx, S.n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return maha ? gicp_fetch9(h, h->gicp.maha, S.pitch, S.n, maha) : (int)MI355NDT_OK;
}

// ---- cost ---------------------------------------------------------------------------------------------
// the thirteen sums over the resident correspondences at applyState(base, x): one sweep, one wait, the record read from mapped memory
static int gicp_sums(mi355ndt_handle* h, const char* where, const double x[6], const float* base, double sums[GC_SUMS]) {
  auto& gc = h->gicp;
  if (!gc.have_corr) { h->err = std::string(where) + ": no correspondences are resident (mi355ndt_gicp_correspondences first)"; return MI355NDT_ERR_STATE; }
  GicpView S, D;
  int rc = gicp_view(h, MI355NDT_GICP_TARGET, where, &D);
  if (!rc) rc = gicp_view(h, MI355NDT_GICP_SOURCE, where, &S);
  if (rc) return rc;
  hipStream_t s = h->stream;
  const unsigned chunks = (unsigned)((S.n + GC_CHUNK - 1) / GC_CHUNK);
  HIPCHK(h, gc.part.reserve((size_t)chunks * GC_SUMS));
  if (!gc.h_rec) {
    HIPCHK(h, gc.h_rec.reserve(GC_REC, hipHostMallocMapped));
    gc.d_rec = gc.h_rec.dev();
    if (!gc.d_rec) { h->err = std::string(where) + ": no device view of the mapped result record"; return MI355NDT_ERR_HIP; }
  }
  const GcCost a = gicp_make_cost(x, base);
  k_gc_cost<<<chunks, GC_CHUNK, 0, s>>>(S.rows, S.pitch, (int)S.n, D.rows, D.pitch, gc.idx, gc.maha, a, gc.part);
  k_gc_cost_final<<<1, 256, 0, s>>>(gc.part, (int)chunks, gc.m, gc.d_rec);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(s));
  for (int k = 0; k < GC_SUMS; k++) sums[k] = gc.h_rec[k];
  return MI355NDT_OK;
}

// computeRDerivative (:134-187); matricesInnerProd (gicp_omp.h:320-329): r += mat1(j, i) * mat2(i, j), i outer
static void gicp_r_derivative(const double x[6], const double R[9], double g[6]) {
  const double phi = x[3], theta = x[4], psi = x[5];
  const double cphi = cos(phi), sphi = sin(phi), ctheta = cos(theta), stheta = sin(theta), cpsi = cos(psi), spsi = sin(psi);
  const double dphi[9] = {0., sphi * spsi + cphi * cpsi * stheta, cphi * spsi - cpsi * sphi * stheta,
                          0., -cpsi * sphi + cphi * spsi * stheta, -cphi * cpsi - sphi * spsi * stheta,
                          0., cphi * ctheta, -ctheta * sphi};
  const double dtheta[9] = {-cpsi * stheta, cpsi * ctheta * sphi, cphi * cpsi * ctheta,
                            -spsi * stheta, ctheta * sphi * spsi, cphi * ctheta * spsi,
                            -ctheta, -sphi * stheta, -cphi * stheta};
  const double dpsi[9] = {-ctheta * spsi, -cphi * cpsi - sphi * spsi * stheta, cpsi * sphi - cphi * spsi * stheta,
                          cpsi * ctheta, -cphi * spsi + cpsi * sphi * stheta, sphi * spsi + cphi * cpsi * stheta,
                          0., 0., 0.};
  const double* D[3] = {dphi, dtheta, dpsi};
  for (int a = 0; a < 3; a++) {
    double r = 0.;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) r += D[a][3 * j + i] * R[3 * i + j];
    g[3 + a] = r;
  }
}

// fdf (:343-378) from the sums: f /= m, g_t *= 2/m, R *= 2/m, computeRDerivative
static void gicp_fdf_sums(const double sums[GC_SUMS], int m, const double x[6], double* f, double* g) {
  if (f) *f = sums[0] / (double)m;
  if (g) {
    const double w = 2.0 / m;
    double R[9];
    for (int k = 0; k < 3; k++) g[k] = sums[1 + k] * w;
    for (int k = 0; k < 9; k++) R[k] = sums[4 + k] * w;
    gicp_r_derivative(x, R, g);
  }
}
static int gicp_fdf(mi355ndt_handle* h, const char* where, const double x[6], const float* base, double* f, double* g) {
  double sums[GC_SUMS];
  int rc = gicp_sums(h, where, x, base, sums);
  if (rc) return rc;
  const int m = h->gicp.n_matched;
  if (m < 1) { h->err = std::string(where) + ": no point is matched"; return MI355NDT_ERR_STATE; }
  gicp_fdf_sums(sums, m, x, f, g);
  return MI355NDT_OK;
}

int mi355ndt_gicp_cost(mi355ndt_handle* h, const double* x, const float* base_colmajor, double* f, double* g) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!x || !base_colmajor) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  return gicp_fdf(h, "gicp_cost", x, base_colmajor, f, g);
}

// ---- align --------------------------------------------------------------------------------------------
// The outer loop of computeTransformation (:415-504) with its BFGS driver, over an evaluator of the two device requests:
//   int match(const float* G, const float* T, int* m)                        one matching pass with transformation_ = T; *m = the matches
//   int sums(const double x[6], const float* base, double sums[GC_SUMS])     the thirteen sums at applyState(base, x)
// (a non-zero return ends the align with that code).  The single-pair surface evaluates on the spot (GicpEvalNow); a slot of
// mi355ndt_gicp_batch_align posts the request to the lockstep round (ndt_host_gicp_batch.hpp).  One copy, so both give the same bytes.
template <typename Eval>
struct GicpFunctor {                               // OptimizationFunctorWithIndices over the sums; a failed evaluation is remembered
  Eval& ev; const float* base; int m; int rc = MI355NDT_OK;
  void eval(const double* x, double* f, double* g) {
    double sums[GC_SUMS];
    const int r = ev.sums(x, base, sums);
    if (r) { if (!rc) rc = r; for (int k = 0; k < GC_SUMS; k++) sums[k] = 0.0; }
    gicp_fdf_sums(sums, m, x, f, g);
  }
  void fdf(const double* x, double& f, double* g) { eval(x, &f, g); }
  double f(const double* x) { double v = 0.0; eval(x, &v, nullptr); return v; }
  void df(const double* x, double* g) { eval(x, nullptr, g); }
};

template <typename Eval>
static int gicp_outer(Eval& ev, const mi355ndt_gicp_params& p, const float* G, float F[16], mi355ndt_gicp_result* result) {
  float T[16], prev[16];
  memcpy(T, GICP_IDENTITY, sizeof T);
  memcpy(prev, T, sizeof T);
  int nr = 0, status = gicp_bfgs::NotStarted, m = 0;
  bool converged = false;
  double delta = 0.0;
  while (!converged) {                            // computeTransformation (:415-504)
    int rc = ev.match(G, T, &m);
    if (rc) return rc;
    memcpy(prev, T, sizeof T);
    if (m < 4) break;                             // NotEnoughPointsException (:197-202): caught, the loop ends unconverged
    double x[6] = {(double)T[12], (double)T[13], (double)T[14],                         // (:204-210) angles in f64 from the f32 entries
                   atan2((double)T[1 * 4 + 2], (double)T[2 * 4 + 2]), asin(-(double)T[0 * 4 + 2]), atan2((double)T[0 * 4 + 1], (double)T[0])};
    GicpFunctor<Eval> fn{ev, G, m};
    gicp_bfgs::BFGS<GicpFunctor<Eval>> bfgs(fn);
    int inner = 0;
    status = gicp_bfgs::minimize(bfgs, x, 1e-2, p.max_inner_iterations, &inner);
    if (fn.rc) return fn.rc;
    if (!gicp_bfgs::accepted(status, inner, p.max_inner_iterations)) break;             // SolverDidntConvergeException: caught likewise
    memcpy(T, GICP_IDENTITY, sizeof T);
    gicp_apply_state(T, x);
    delta = 0.;
    for (int k = 0; k < 4; k++)
      for (int l = 0; l < 4; l++) {
        const double ratio = (k < 3 && l < 3) ? 1. / p.rotation_epsilon : 1. / p.transformation_epsilon;
        const double c_delta = ratio * (double)std::fabs(prev[l * 4 + k] - T[l * 4 + k]);
        if (c_delta > delta) delta = c_delta;
      }
    nr++;
    if (nr >= p.max_iterations || delta < 1) {
      converged = true;
      memcpy(prev, T, sizeof T);
    }
  }
  memcpy(F, GICP_IDENTITY, sizeof T);             // final = [R_t R_g | t_t + t_g] (:508-511)
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) F[c * 4 + r] = (prev[0 * 4 + r] * G[c * 4 + 0] + prev[1 * 4 + r] * G[c * 4 + 1]) + prev[2 * 4 + r] * G[c * 4 + 2];
    F[3 * 4 + r] = prev[3 * 4 + r] + G[3 * 4 + r];
  }
  memcpy(result->final_colmajor, F, sizeof T);
  result->converged = converged ? 1 : 0; result->iterations = nr; result->inner_status = status;
  result->n_matched = m; result->delta = delta;
  return MI355NDT_OK;
}

// the single-pair surface's evaluator: each request is launched and waited for where it is made
struct GicpEvalNow {
  mi355ndt_handle* h;
  int match(const float* G, const float* T, int* m) { const int rc = gicp_match(h, "gicp_align", G, T); *m = h->gicp.n_matched; return rc; }
  int sums(const double* x, const float* base, double* sums) { return gicp_sums(h, "gicp_align", x, base, sums); }
};

int mi355ndt_gicp_align(mi355ndt_handle* h, const float* guess_colmajor, mi355ndt_gicp_result* result) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!guess_colmajor || !result) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  auto& gc = h->gicp;
  gc.have_final = false;
  GicpEvalNow ev{h};
  mi355ndt_gicp_result r;
  const int rc = gicp_outer(ev, gc.prm, guess_colmajor, gc.final_cm, &r);
  if (rc) return rc;
  gc.have_final = true;
  *result = r;
  return MI355NDT_OK;
}

// a cloud moved by F (column-major) into the caller's records
static int gicp_move_out(mi355ndt_handle* h, const GicpView& S, const float* F, void* out_pts, size_t out_stride_bytes) {
  auto& gc = h->gicp;
  if (S.n == 0) return MI355NDT_OK;
  HIPCHK(h, gc.moved.reserve(3 * S.n));
  GcCost a;
  memcpy(a.Tx, F, sizeof a.Tx); memcpy(a.B, F, sizeof a.B);
  k_gc_move<<<(unsigned)((S.n + 255) / 256), 256, 0, h->stream>>>(S.rows, S.pitch, (int)S.n, a, gc.moved);
  HIPCHK(h, hipGetLastError());
  std::vector<float> tmp(3 * S.n);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), gc.moved, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned char* o = (unsigned char*)out_pts;
  for (size_t i = 0; i < S.n; i++) memcpy(o + i * out_stride_bytes, &tmp[3 * i], 12);
  return MI355NDT_OK;
}

int mi355ndt_gicp_get_aligned(mi355ndt_handle* h, void* out_pts, size_t out_stride_bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!out_pts || out_stride_bytes < 12) return MI355NDT_ERR_BAD_ARG;
  auto& gc = h->gicp;
  if (!gc.have_final) { h->err = "gicp_get_aligned: no align has run"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  GicpView S;
  int rc = gicp_view(h, MI355NDT_GICP_SOURCE, "gicp_get_aligned", &S);
  if (rc) return rc;
  return gicp_move_out(h, S, gc.final_cm, out_pts, out_stride_bytes);
}
