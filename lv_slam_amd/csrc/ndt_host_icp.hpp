// ndt_host_icp.hpp -- mi355ndt_icp_*: pcl::IterativeClosestPoint for one pair, synchronously (kernels: ndt_icp.hpp; the estimate, the
// criteria and the loop: icp_outer.hpp).  The host holds the parameters, the two clouds and the working cloud; an iteration is two launches
// (k_icp_step, k_icp_final) and one wait, and the record is read from mapped memory.  Clouds are GicpSide / GicpView (ndt_host_gicp.hpp); the
// target's index is built by gicp_prepare_index on first use (a keyframe's is the one the fitness scores and GICP search), without
// covariances; a source needs no index.  The GICP surface, the batches, the grids, the keyframes' rows and the other workspaces are left as
// they were.  The pieces the batch form shares (ndt_host_icp_batch.hpp): icp_views, icp_work_reserve, icp_make_step, icp_work_out.
#pragma once

int mi355ndt_icp_params_default(mi355ndt_icp_params* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  p->transformation_epsilon = 0.0; p->max_iterations = 10; p->euclidean_fitness_epsilon = -DBL_MAX;   // pcl::Registration's constructor
  p->corr_dist_threshold = std::sqrt(DBL_MAX); p->min_number_correspondences = 3; p->use_reciprocal_correspondences = 0;
  return MI355NDT_OK;
}

int mi355ndt_icp_set_params(mi355ndt_handle* h, const mi355ndt_icp_params* p) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!p) return MI355NDT_ERR_BAD_ARG;
  if (p->use_reciprocal_correspondences) {
    h->err = "icp_set_params: use_reciprocal_correspondences is not served (it needs a search over the moving cloud every iteration)";
    return MI355NDT_ERR_BAD_ARG;
  }
  if (!(p->transformation_epsilon >= 0) || !(p->corr_dist_threshold >= 0) || p->euclidean_fitness_epsilon != p->euclidean_fitness_epsilon) {
    h->err = "icp_set_params: an epsilon or the correspondence distance is NaN or negative"; return MI355NDT_ERR_BAD_ARG;
  }
  if (p->max_iterations < 0 || p->min_number_correspondences < 0) { h->err = "icp_set_params: a negative iteration or correspondence count"; return MI355NDT_ERR_BAD_ARG; }
  h->icp.prm = *p;
  return MI355NDT_OK;
}

// ---- the two clouds -----------------------------------------------------------------------------------
static int icp_set_host(mi355ndt_handle* h, int role, const void* pts, size_t n, size_t stride) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  const int rc = gicp_side_set_host(h, h->icp.side[role], pts, n, stride);
  if (rc != MI355NDT_ERR_BAD_ARG) h->icp.work.have_final = false;   // (refused arguments change nothing)
  return rc;
}
static int icp_set_keyframe(mi355ndt_handle* h, int role, int id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!kf_find(h, id, role == MI355NDT_GICP_TARGET ? "icp_set_target_keyframe" : "icp_set_source_keyframe")) return MI355NDT_ERR_BAD_ARG;
  GicpSide& sd = h->icp.side[role];
  sd.kf_id = id; sd.set = true;
  h->icp.work.have_final = false;
  return MI355NDT_OK;
}
int mi355ndt_icp_set_target(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes) { return icp_set_host(h, MI355NDT_GICP_TARGET, pts, n, stride_bytes); }
int mi355ndt_icp_set_source(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes) { return icp_set_host(h, MI355NDT_GICP_SOURCE, pts, n, stride_bytes); }
int mi355ndt_icp_set_target_keyframe(mi355ndt_handle* h, int id) { return icp_set_keyframe(h, MI355NDT_GICP_TARGET, id); }
int mi355ndt_icp_set_source_keyframe(mi355ndt_handle* h, int id) { return icp_set_keyframe(h, MI355NDT_GICP_SOURCE, id); }

// the target with its index, ready to be searched; waits for the device
static int icp_target(mi355ndt_handle* h, const char* where, GicpView* D) {
  int rc = gicp_view_side(h, h->icp.side[MI355NDT_GICP_TARGET], where, ": no target cloud is set", D);
  if (rc) return rc;
  if (D->n == 0) { h->err = std::string(where) + ": the target cloud is empty"; return MI355NDT_ERR_BAD_ARG; }
  return gicp_prepare_index(h, *D);
}
// a source and the working cloud's buffers for it
static int icp_source(mi355ndt_handle* h, GicpSide& sd, mi355ndt_handle::IcpWork& w, const char* where, const char* unset, GicpView* S) {
  int rc = gicp_view_side(h, sd, where, unset, S);
  if (rc) return rc;
  if (S->n == 0) { h->err = std::string(where) + ": the source cloud is empty"; return MI355NDT_ERR_BAD_ARG; }
  rc = uploads_before_compute(h);                 // (a keyframe_add's transfer may still be on its way)
  if (rc) return rc;
  w.have_final = false;
  HIPCHK(h, w.W.reserve(3 * S->pitch)); HIPCHK(h, w.d2.reserve(S->pitch)); HIPCHK(h, w.idx.reserve(S->pitch));
  HIPCHK(h, w.part.reserve((S->n + GC_CHUNK - 1) / GC_CHUNK * ICP_SUMS));
  w.n = S->n; w.pitch = S->pitch;
  return MI355NDT_OK;
}

// what a step takes to the device (host arithmetic only): moves = 2: T (G p) from the source rows, 1: T alone
static IcpStep icp_make_step(const mi355ndt_icp_params& p, const float* G, const float* T) {
  IcpStep a;
  memcpy(a.G, G ? G : ICP_IDENTITY, sizeof a.G); memcpy(a.T, T, sizeof a.T);
  a.moves = G ? 2 : 1;
  a.thr2 = p.corr_dist_threshold * p.corr_dist_threshold;
  a.range = (float)a.thr2;                         // the f32 just above thr2 (inf when thr2 is beyond f32): what lies further cannot match
  if ((double)a.range <= a.thr2) a.range = nextafterf(a.range, INFINITY);
  return a;
}

static int icp_record(mi355ndt_handle* h, const char* where) {
  auto& ic = h->icp;
  if (!ic.h_rec) {
    HIPCHK(h, ic.h_rec.reserve(ICP_REC, hipHostMallocMapped));
    ic.d_rec = ic.h_rec.dev();
    if (!ic.d_rec) { ic.h_rec = PinBuf<double>(); h->err = std::string(where) + ": no device view of the mapped result record"; return MI355NDT_ERR_HIP; }
  }
  HIPCHK(h, ic.m.reserve(1));
  HIPCHK(h, hipMemsetAsync(ic.m, 0, sizeof(int), h->stream));   // (a failed step may have left a count behind)
  return MI355NDT_OK;
}

// one step of the surface's pair: two launches, one wait
static int icp_step_now(mi355ndt_handle* h, const GicpView& S, const GicpView& D, bool from_source, const IcpStep& a, IcpSums* out) {
  auto& ic = h->icp;
  auto& w = ic.work;
  hipStream_t s = h->stream;
  const unsigned chunks = (unsigned)((S.n + GC_CHUNK - 1) / GC_CHUNK);
  k_icp_step<<<chunks, GC_CHUNK, 0, s>>>(from_source ? S.rows : (const float*)w.W, w.W, S.pitch, (int)S.n, kfi_view(*D.index, D.rows, D.pitch, D.n), a,
                                        w.idx, w.d2, w.part, ic.m);
  k_icp_final<<<1, 256, 0, s>>>(w.part, (int)chunks, ic.m, ic.d_rec);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(s));
  for (int k = 0; k < ICP_SUMS; k++) out->v[k] = ic.h_rec[k];
  out->m = (int)ic.h_rec[ICP_SUMS];
  return MI355NDT_OK;
}

int mi355ndt_icp_correspondences(mi355ndt_handle* h, const float* guess_colmajor, const float* T_colmajor, int* idx, float* d2, double* sums, int* m) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!guess_colmajor) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  auto& ic = h->icp;
  GicpView S, D;
  int rc = icp_target(h, "icp_correspondences", &D);
  if (!rc) rc = icp_source(h, ic.side[MI355NDT_GICP_SOURCE], ic.work, "icp_correspondences", ": no source cloud is set", &S);
  if (!rc) rc = icp_record(h, "icp_correspondences");
  if (rc) return rc;
  IcpSums out;
  rc = icp_step_now(h, S, D, true, icp_make_step(ic.prm, guess_colmajor, T_colmajor ? T_colmajor : ICP_IDENTITY), &out);
  if (rc) return rc;
  if (m) *m = out.m;
  if (sums) memcpy(sums, out.v, sizeof out.v);
  if (idx) HIPCHK(h, hipMemcpyAsync(idx, ic.work.idx, S.n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (d2) HIPCHK(h, hipMemcpyAsync(d2, ic.work.d2, S.n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MI355NDT_OK;
}

// ---- align --------------------------------------------------------------------------------------------
// the single-pair surface's evaluator of icp_outer: the one run's step is launched and waited for where it is asked
struct IcpEvalNow {
  mi355ndt_handle* h; const GicpView& S; const GicpView& D;
  int step(const int*, int, const IcpRun* runs, IcpSums* sums) {
    return icp_step_now(h, S, D, runs[0].first, icp_make_step(h->icp.prm, nullptr, runs[0].T), &sums[0]);
  }
};

int mi355ndt_icp_align(mi355ndt_handle* h, const float* guess_colmajor, mi355ndt_icp_result* result) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!guess_colmajor || !result) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  auto& ic = h->icp;
  GicpView S, D;
  int rc = icp_target(h, "icp_align", &D);
  if (!rc) rc = icp_source(h, ic.side[MI355NDT_GICP_SOURCE], ic.work, "icp_align", ": no source cloud is set", &S);
  if (!rc) rc = icp_record(h, "icp_align");
  if (rc) return rc;
  IcpEvalNow ev{h, S, D};
  std::vector<IcpRun> runs;
  rc = icp_outer(ev, ic.prm, 1, guess_colmajor, runs, nullptr, nullptr);
  if (rc) return rc;
  ic.work.run = runs[0];
  ic.work.have_final = true;
  icp_result(runs[0], result);
  return MI355NDT_OK;
}

// a working cloud after its run, the pending last move applied on the way out, into the caller's records
static int icp_work_out(mi355ndt_handle* h, const mi355ndt_handle::IcpWork& w, void* out_pts, size_t out_stride_bytes) {
  auto& ic = h->icp;
  HIPCHK(h, ic.moved.reserve(3 * w.n));
  IcpStep a = icp_make_step(ic.prm, nullptr, w.run.T);
  a.moves = w.run.pending ? 1 : 0;
  k_icp_out<<<(unsigned)((w.n + 255) / 256), 256, 0, h->stream>>>(w.W, w.pitch, (int)w.n, a, ic.moved);
  HIPCHK(h, hipGetLastError());
  std::vector<float> tmp(3 * w.n);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), ic.moved, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned char* o = (unsigned char*)out_pts;
  for (size_t i = 0; i < w.n; i++) memcpy(o + i * out_stride_bytes, &tmp[3 * i], 12);
  return MI355NDT_OK;
}

int mi355ndt_icp_get_aligned(mi355ndt_handle* h, void* out_pts, size_t out_stride_bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!out_pts || out_stride_bytes < 12) return MI355NDT_ERR_BAD_ARG;
  if (!h->icp.work.have_final) { h->err = "icp_get_aligned: no align has run"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return icp_work_out(h, h->icp.work, out_pts, out_stride_bytes);
}
