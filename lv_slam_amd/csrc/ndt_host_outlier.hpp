// ndt_host_outlier.hpp -- mi355ndt_prefilter_outliers: PrefilteringNodelet::outlier_removal (prefiltering_nodelet.cpp:128, 150-161) over the
// resident prefilter result, in place (ndt_outlier.hpp).  The index (a CloudIndex, rebuilt by every call), dist[] and its pinned twin are this
// surface's own; the index build's sort, the flags, the scan and the compaction target use the shared scratch (h->vs).  The batch, the
// grids, the keyframes and their indexes, the map-cloud and window workspaces are left as they were.
#pragma once

int mi355ndt_outlier_params_default(mi355ndt_outlier_params* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  p->method = MI355NDT_OUTLIER_STATISTICAL;
  p->mean_k = 20; p->stddev_mul = 1.0;            // prefiltering_nodelet.cpp:63-64
  p->radius = 0.8; p->min_neighbors = 2;          // (:72-73)
  return MI355NDT_OK;
}

// StatisticalOutlierRemoval's statistics: f64, strictly in index order over every dist[i], the zeros of the non-valid points included
static void outlier_statistics(const float* dist, size_t n, long long n_valid, double stddev_mul, mi355ndt_outlier_stats* st) {
  double sum = 0.0, sq = 0.0;
  for (size_t i = 0; i < n; i++) { const double d = (double)dist[i]; sum += d; sq += d * d; }
  const double nv = (double)n_valid;
  const double mean = sum / nv;
  const double var = (sq - sum * sum / nv) / (nv - 1.0);
  const double stddev = std::sqrt(var);
  st->n_in = (long long)n; st->n_valid = n_valid;
  st->mean = mean; st->stddev = stddev; st->threshold = mean + stddev_mul * stddev;
}

template <int CAP>
static void outlier_knn_launch(hipStream_t s, unsigned blocks, const KfiView& v, int method, int K, float r2, float* dist, int* keep) {
  k_ol_knn<CAP><<<blocks, OL_LANES, 0, s>>>(v, method, K, r2, dist, keep);
  k_ol_knn_brute<CAP><<<blocks, OL_LANES, 0, s>>>(v, method, K, r2, dist, keep);   // (the kernels decide by the lattice's status)
}

int mi355ndt_prefilter_outliers(mi355ndt_handle* h, const mi355ndt_outlier_params* p, float* mean_distances,
                                void* out_pts, size_t out_capacity, size_t out_stride, size_t* n_out, mi355ndt_outlier_stats* stats) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!p || !n_out || (out_pts && out_stride < 12)) return MI355NDT_ERR_BAD_ARG;
  const bool statistical = p->method == MI355NDT_OUTLIER_STATISTICAL;
  if (!statistical && p->method != MI355NDT_OUTLIER_RADIUS) { h->err = "prefilter_outliers: unknown method"; return MI355NDT_ERR_BAD_ARG; }
  if ((p->mean_k < 1 || p->mean_k > OL_MAX_K)) { h->err = "prefilter_outliers: mean_k outside 1..64"; return MI355NDT_ERR_BAD_ARG; }
  if (std::isnan(p->stddev_mul)) { h->err = "prefilter_outliers: stddev_mul is NaN"; return MI355NDT_ERR_BAD_ARG; }
  if ((p->min_neighbors < 0 || p->min_neighbors > OL_MAX_K)) { h->err = "prefilter_outliers: min_neighbors outside 0..64"; return MI355NDT_ERR_BAD_ARG; }
  if (!(p->radius >= 0.0)) { h->err = "prefilter_outliers: radius is NaN or negative"; return MI355NDT_ERR_BAD_ARG; }
  if (!h->d_pf_out) { h->err = "prefilter_outliers: no prefilter result is resident (mi355ndt_prefilter first)"; return MI355NDT_ERR_STATE; }
  *n_out = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  const size_t n = (size_t)h->pf_count, pitch = h->pf_pitch;
  if (n == 0) return MI355NDT_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int method = statistical ? OL_STATISTICAL : OL_RADIUS;
  const int K = statistical ? p->mean_k : p->min_neighbors;
  const float r2 = (float)(p->radius * p->radius);
  VoxelScratch& w = h->vs;
  VsNeed need;
  need.pitch = pitch; need.x = 3 * pitch; need.stat = 2;
  int rc = vs_reserve(h, need);
  if (rc) return rc;
  HIPCHK(h, h->d_ol_dist.reserve(pitch));
  HIPCHK(h, h->h_ol_dist.reserve(pitch));
  float* rows = h->d_pf_out;
  const int gx = (int)((pitch + 255) / 256);
  HIPCHK(h, hipMemsetAsync(h->d_ol_dist, 0, pitch * sizeof(float), s));
  HIPCHK(h, hipMemsetAsync(w.flag, 0, pitch * sizeof(int), s));
  if (K > 0) {                                    // (w.stat[0], [1]: the lattice's status and the number of searchable points)
    rc = kfi_build_rows(h, rows, pitch, n, h->ol_cell_mm, h->ol_index, 0);
    if (rc) return rc;
    const KfiView v = kfi_view(h->ol_index, rows, pitch, n);
    const unsigned blocks = (unsigned)((n + OL_LANES - 1) / OL_LANES);
    if (K <= 32) outlier_knn_launch<32>(s, blocks, v, method, K, r2, h->d_ol_dist, w.flag);
    else outlier_knn_launch<64>(s, blocks, v, method, K, r2, h->d_ol_dist, w.flag);
    HIPCHK(h, hipGetLastError());
  } else {                                        // RADIUS with min_neighbors = 0: every searchable point is kept
    k_ol_finite<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(rows, pitch, (int)n, w.flag);
  }
  if (statistical) {
    // the index-order f64 sums are two dependent chains over n values: dist[] comes back once, the host forms the threshold, and the
    // threshold goes to the flag kernel as an argument (the first of the call's two waits)
    HIPCHK(h, hipMemcpyAsync(h->h_ol_dist, h->d_ol_dist, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(w.h_ret, w.stat, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    const long long nf = (long long)w.h_ret[1];
    mi355ndt_outlier_stats st;
    outlier_statistics(h->h_ol_dist, n, nf >= (long long)K + 1 ? nf : 0, p->stddev_mul, &st);
    if (stats) *stats = st;
    if (mean_distances) memcpy(mean_distances, h->h_ol_dist, n * sizeof(float));
    k_ol_flag<<<gx, 256, 0, s>>>(h->d_ol_dist, (int)n, pitch, st.threshold, w.flag);
  } else if (mean_distances) {
    memset(mean_distances, 0, n * sizeof(float));
  }
  exscan_ints(s, w.flag, pitch, w.tmp, w.pos);
  HIPCHK(h, hipMemsetAsync(w.x, 0, 3 * pitch * sizeof(float), s));
  k_ol_compact<<<gx, 256, 0, s>>>(rows, pitch, w.flag, w.pos, w.x);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(rows, w.x, 3 * pitch * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(h, hipMemcpyAsync(w.h_ret, w.pos + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(w.h_ret + 1, w.flag + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  const size_t m = (size_t)w.h_ret[0] + (size_t)w.h_ret[1];
  h->pf_count = (int)m;
  *n_out = m;
  if (out_pts) {
    if (m > out_capacity) return MI355NDT_ERR_BAD_ARG;
    std::vector<float> tmp(3 * pitch);
    HIPCHK(h, hipMemcpy(tmp.data(), rows, 3 * pitch * sizeof(float), hipMemcpyDeviceToHost));
    rows_to_records(tmp.data(), pitch, 3, m, out_pts, out_stride, -1);
  }
  return MI355NDT_OK;
}
