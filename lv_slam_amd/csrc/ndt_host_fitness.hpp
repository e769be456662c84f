// ndt_host_fitness.hpp -- getFitnessScore for one pair and for every batch slot (one function), calculateScore.
#pragma once

// ---- shared by the single, the batch and the keyframe fitness calls ---------------------------------------
// max_range as the kernels take it
static float fit_range_f32(double max_range) { return max_range >= 3.0e38 ? 3.0e38f : (float)max_range; }

// the block partials (sum, count) of one pair or edge, added on the host in block order from 0.0
static void fit_reduce(const double* part, int nblk, double* score, long long* n_inliers) {
  double sum = 0, cnt = 0;
  for (int k = 0; k < nblk; k++) { sum += part[2 * (size_t)k]; cnt += part[2 * (size_t)k + 1]; }
  *score = cnt > 0 ? sum / cnt : 1.7976931348623157e308;     // std::numeric_limits<double>::max()
  if (n_inliers) *n_inliers = (long long)cnt;
}

// getFitnessScore(max_range) of every slot of the batch the handle holds -- one slot on the single-registration surface.  T: B column-major
// transforms on the host, or null = the final poses the last align left in d_results (the identity before any).  The callers have checked
// their arguments and the handle's state.  Per pair: the block partials of k_fitness_batch (a grid) or k_fitness_brute_batch (none), summed
// on the host in block order from 0.0; no point to score on either side, or none finite in the target (GRID_EMPTY): (DBL_MAX, 0), no launch.
static int fit_scores(mi355ndt_handle* h, const float* T, double max_range, double* scores, long long* n_inliers) {
  { int rc = ensure_grids(h, GRIDS_ANY); if (rc) return rc; }
  const int B = h->n_pairs;
  const size_t tp = h->tgt_pitch;
  hipStream_t s = h->stream;
  std::vector<GridDesc> gd(B);
  HIPCHK(h, hipMemcpyAsync(gd.data(), h->d_grid, (size_t)B * sizeof(GridDesc), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  const float mr = fit_range_f32(max_range);
  std::vector<int> part0(B, 0), nblk(B, 0);
  int n_part = 0;
  // the index covers EVERY pair with a grid, whatever its source holds now (k_fit_* index every GRID_OK pair, and a source set later
  // does not rebuild it): the pool is sized over all of them
  size_t total_words = 0;
  bool any_ok = false;
  for (int b = 0; b < B; b++) {
    if (gd[b].status != GRID_OK) continue;
    any_ok = true;
    total_words = std::max(total_words, (size_t)gd[b].word_off + (size_t)gd[b].nwords);
  }
  for (int b = 0; b < B; b++) {
    const int ns = h->h_src_cnt[b];
    if (gd[b].status == GRID_EMPTY || ns <= 0) continue;
    nblk[b] = (ns + 255) / 256;
    part0[b] = n_part;
    n_part += nblk[b];
  }
  if (any_ok && !h->built.fit_index) {
    HIPCHK(h, h->d_fwords.reserve(total_words));
    HIPCHK(h, h->d_fruns.reserve((size_t)B * (tp + 1)));
    HIPCHK(h, hipMemsetAsync(h->d_fwords, 0, total_words * sizeof(BitWord), s));
    const dim3 pg((unsigned)((tp + 255) / 256), (unsigned)B);
    k_fit_mark<<<pg, 256, 0, s>>>(h->d_keys_b, tp, h->d_grid, h->d_fwords, h->built.cb);
    k_fit_rank<<<B, 1024, 0, s>>>(h->d_grid, h->d_fwords);
    k_fit_runs<<<pg, 256, 0, s>>>(h->d_keys_b, tp, h->d_grid, h->d_fwords, h->d_fruns, h->built.cb);
    HIPCHK(h, hipGetLastError());
    h->built.fit_index = true;
  }
  // item tables of the two launches: a grid -> k_fitness_batch, no grid (a target without one has no leaf size either) -> k_fitness_brute_batch
  std::vector<int> tab, tab_brute;
  int gmax = 0, gmax_brute = 0;
  for (const bool with_grid : {true, false})
    fit_item_table(B, nblk, part0, [&](int b) { return (gd[b].status == GRID_OK) == with_grid; },
                   [&](int b) { return std::array<int, 3>{h->h_src_cnt[b], h->h_tgt_cnt[b], with_grid ? fit_ring_max(max_range, gd[b].leaf) : 0}; },
                   with_grid ? tab : tab_brute, with_grid ? gmax : gmax_brute);
  const size_t brute_at = tab.size();
  tab.insert(tab.end(), tab_brute.begin(), tab_brute.end());
  const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float* dT = nullptr;
  int Tstride = 16;
  if (n_part > 0) {
    static_assert(sizeof(mi355ndt_result) % sizeof(float) == 0 && offsetof(mi355ndt_result, final_colmajor) == 0, "final pose at the head of a result");
    if (T) {
      HIPCHK(h, h->d_fit_T.reserve((size_t)B * 16));
      HIPCHK(h, hipMemcpyAsync(h->d_fit_T, T, (size_t)B * 16 * sizeof(float), hipMemcpyHostToDevice, s));
      dT = h->d_fit_T;
    } else if (h->aligned_once) {                  // read where the align left them, no host round trip
      dT = reinterpret_cast<const float*>(h->d_results.p);
      Tstride = (int)(sizeof(mi355ndt_result) / sizeof(float));
    } else {
      HIPCHK(h, h->d_fit_T.reserve(16));
      HIPCHK(h, hipMemcpyAsync(h->d_fit_T, ident, sizeof ident, hipMemcpyHostToDevice, s));
      dT = h->d_fit_T;
      Tstride = 0;
    }
    HIPCHK(h, h->d_fit_items.reserve(tab.size()));
    HIPCHK(h, hipMemcpyAsync(h->d_fit_items, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(h, h->d_fit.reserve((size_t)2 * n_part));
    const int* t_ok = h->d_fit_items;
    const int* t_brute = h->d_fit_items + brute_at;
    if (gmax) k_fitness_batch<<<8u * (unsigned)gmax, 256, 0, s>>>(reinterpret_cast<const FitItem*>(t_ok + 16), t_ok, h->d_src, h->src_pitch, h->d_tgt, tp,
                                                                h->d_vals_b, h->d_grid, h->d_fwords, h->d_fruns, dT, Tstride, mr, h->d_fit);
    if (gmax_brute) k_fitness_brute_batch<<<8u * (unsigned)gmax_brute, 256, 0, s>>>(reinterpret_cast<const FitItem*>(t_brute + 16), t_brute, h->d_src, h->src_pitch,
                                                                                  h->d_tgt, tp, dT, Tstride, mr, h->d_fit);
    HIPCHK(h, hipGetLastError());
  }
  std::vector<double> part((size_t)2 * n_part);
  if (n_part > 0) HIPCHK(h, hipMemcpyAsync(part.data(), h->d_fit, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  for (int b = 0; b < B; b++) fit_reduce(part.data() + 2 * (size_t)part0[b], nblk[b], scores + b, n_inliers ? n_inliers + b : nullptr);
  return MI355NDT_OK;
}

// replaces pcl::Registration::getFitnessScore(max_range) for the loop-closure caller (loop_detector.hpp:249-262): the batch of one
int mi355ndt_fitness_score_T(mi355ndt_handle* h, const float T_colmajor[16], double max_range, double* score, long long* n_inliers) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!T_colmajor || !score) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs != 1 || !h->have_target || !h->have_source) return MI355NDT_ERR_STATE;
  if (h->h_tgt_cnt[0] <= 0 || h->h_src_cnt[0] <= 0) return MI355NDT_ERR_STATE;
  return fit_scores(h, T_colmajor, max_range, score, n_inliers);
}

int mi355ndt_get_fitness_score(mi355ndt_handle* h, double max_range, double* score, long long* n_inliers) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  return mi355ndt_fitness_score_T(h, h->last_final, max_range, score, n_inliers);
}

// getFitnessScore(max_range) for every batch slot (include/mi355_ndt.h).  An empty source or target scores (DBL_MAX, 0) here; the
// one-pair call refuses it (MI355NDT_ERR_STATE).
int mi355ndt_batch_fitness_scores(mi355ndt_handle* h, const float* T_colmajor, double max_range, double* scores, long long* n_inliers) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!scores) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs <= 0 || !h->d_tgt || !h->d_src) return MI355NDT_ERR_STATE;
  return fit_scores(h, T_colmajor, max_range, scores, n_inliers);
}

// replaces calculateScore(cloud) (ndt_omp.h:232, ndt_omp_impl2.hpp:1006-1040)
int mi355ndt_calculate_score(mi355ndt_handle* h, const void* pts, size_t n, size_t stride, double* score) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!score || (!pts && n) || (n && stride < 12) || n >= (1u << 31)) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs != 1 || !h->have_target || h->h_tgt_cnt[0] <= 0) return MI355NDT_ERR_STATE;
  if (n == 0) { *score = std::nan(""); return MI355NDT_OK; }                     // 0 / 0 in the reference
  int rc = ensure_grids(h, GRIDS_LIVE);
  if (rc) return rc;
  const size_t pitch = (n + 63) & ~(size_t)63;
  HIPCHK(h, h->d_score_pts.reserve(3 * pitch));
  const int blocks = (int)((n + SCORE_THREADS - 1) / SCORE_THREADS);
  HIPCHK(h, h->d_score_part.reserve((size_t)blocks));
  rc = upload_cloud(h, h->d_score_pts, pitch, 0, pts, n, stride);
  if (rc) return rc;
  rc = uploads_before_compute(h);
  if (rc) return rc;
  SweepConst sc;
  make_sweep_const(h, sc);
  hipStream_t s = h->stream;
  k_calc_score<<<blocks, SCORE_THREADS, 0, s>>>(h->d_score_pts, pitch, (int)n, h->d_grid, h->d_words, h->d_recs, h->d_icov64, h->d_cent,
                                                h->gauss_last[0], h->gauss_last[1], h->gauss_last[2], sc.kd_r2, sc.leaf_pow2, sc.inv_leaf, h->d_score_part);
  std::vector<double> part((size_t)blocks);
  HIPCHK(h, hipMemcpyAsync(part.data(), h->d_score_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  double sum = 0;
  for (int b = 0; b < blocks; b++) sum += part[(size_t)b];
  *score = sum / (double)n;                                                      // impl2:1040
  return compute_enqueued(h);
}
