// ndt_host_fitness.hpp -- getFitnessScore for one pair and for every batch slot, calculateScore.
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

// Item table of one launch (FitItem, ndt_fitness.hpp): 16 ints of group starts, then the items group by group.  Item i of N (a pair, an
// edge; nblk[i] blocks of 256 points) takes part iff takes(i), and goes to the least loaded of the eight groups, in index order;
// tail(i) gives the three ints behind {i, first block in its group, part0[i]}.  The order decides which block partial lands where.
template <typename Takes, typename Tail>
static void fit_item_table(int N, const std::vector<int>& nblk, const std::vector<int>& part0, Takes takes, Tail tail, std::vector<int>& t, int& group_max) {
  int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int> group((size_t)N, -1);
  for (int i = 0; i < N; i++) {
    if (nblk[(size_t)i] == 0 || !takes(i)) continue;
    int g = 0;
    for (int k = 1; k < 8; k++) if (load[k] < load[g]) g = k;
    group[(size_t)i] = g;
    load[g] += nblk[(size_t)i];
  }
  t.assign(16, 0);
  for (int g = 0; g < 8; g++) {
    t[(size_t)g] = (int)((t.size() - 16) / 6);
    for (int i = 0, blk = 0; i < N; i++) {
      if (group[(size_t)i] != g) continue;
      const std::array<int, 3> x = tail(i);
      t.insert(t.end(), {i, blk, part0[(size_t)i], x[0], x[1], x[2]});
      blk += nblk[(size_t)i];
    }
  }
  t[8] = (int)((t.size() - 16) / 6);
  group_max = *std::max_element(load, load + 8);
}

// replaces pcl::Registration::getFitnessScore(max_range) for the loop-closure caller (loop_detector.hpp:249-262)
int mi355ndt_fitness_score_T(mi355ndt_handle* h, const float T_colmajor[16], double max_range, double* score, long long* n_inliers) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!T_colmajor || !score) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs != 1 || !h->have_target || !h->have_source) return MI355NDT_ERR_STATE;
  if (h->h_tgt_cnt[0] <= 0 || h->h_src_cnt[0] <= 0) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  { int rcu = uploads_before_compute(h); if (rcu) return rcu; }
  if (!h->targets_built) { int rc = mi355ndt_batch_build_targets(h); if (rc) return rc; }
  hipStream_t s = h->stream;
  GridDesc g;
  HIPCHK(h, hipMemcpyAsync(&g, h->d_grid, sizeof g, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (g.status == GRID_EMPTY) { *score = 1.7976931348623157e308; if (n_inliers) *n_inliers = 0; return MI355NDT_OK; }
  const bool brute = g.status != GRID_OK;        // no voxel grid (leaf-too-small guard / cell cap): the score does not need one
  if (!brute && !h->cells_ready) {
    const size_t nc = (size_t)g.ncells;
    HIPCHK(h, h->d_cstart.reserve(nc)); HIPCHK(h, h->d_cend.reserve(nc));
    HIPCHK(h, hipMemsetAsync(h->d_cstart, 0, nc * sizeof(unsigned), s));
    HIPCHK(h, hipMemsetAsync(h->d_cend, 0, nc * sizeof(unsigned), s));
    k_cellrange<unsigned><<<(unsigned)((h->tgt_pitch + 255) / 256), 256, 0, s>>>(h->d_keys_b, h->tgt_pitch, h->last_cb,
                                                                                h->d_cstart, h->d_cend);
    h->cells_ready = true;
  }
  const int n = h->h_src_cnt[0];
  const int blocks = (n + 255) / 256;
  HIPCHK(h, h->d_fit.reserve((size_t)2 * blocks));
  HIPCHK(h, hipMemcpyAsync(h->d_hook, T_colmajor, 16 * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipStreamSynchronize(s));
  const float mr = fit_range_f32(max_range);
  // rings needed to cover sqrt(max_range) (+1 cell of slack)
  double rr = brute ? 0.0 : std::sqrt(std::min(max_range, 1e30)) / (double)g.leaf + 2.0;   // (a target without a grid has no leaf size to divide by)
  // (a query outside the grid may sit further away than the grid is wide: the kernel clamps its cell to 2^29 cells from the grid's
  //  origin, so 2^30 rings reach every target cell from anywhere)
  const int ring_max = rr > (double)(1 << 30) ? (1 << 30) : (int)rr;
  if (brute) k_fitness_brute<<<blocks, 256, 0, s>>>(h->d_src, h->src_pitch, n, h->d_tgt, h->tgt_pitch, h->h_tgt_cnt[0], h->d_hook, mr, h->d_fit);
  else k_fitness<<<blocks, 256, 0, s>>>(h->d_src, h->src_pitch, n, h->d_tgt, h->tgt_pitch, h->d_vals_b, h->d_grid, h->d_cstart, h->d_cend,
                                        h->d_hook, mr, ring_max, h->d_fit);
  std::vector<double> part((size_t)2 * blocks);
  HIPCHK(h, hipMemcpyAsync(part.data(), h->d_fit, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  fit_reduce(part.data(), blocks, score, n_inliers);
  return MI355NDT_OK;
}

int mi355ndt_get_fitness_score(mi355ndt_handle* h, double max_range, double* score, long long* n_inliers) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  return mi355ndt_fitness_score_T(h, h->last_final, max_range, score, n_inliers);
}

// getFitnessScore(max_range) for every batch slot (include/mi355_ndt.h): per pair, word for word what mi355ndt_fitness_score_T returns on a
// one-pair engine holding the same clouds and transform -- the same block partials (k_fitness_batch / k_fitness_brute_batch), summed on
// the host in block order from 0.0 as there.
int mi355ndt_batch_fitness_scores(mi355ndt_handle* h, const float* T_colmajor, double max_range, double* scores, long long* n_inliers) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!scores) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs <= 0 || !h->d_tgt || !h->d_src) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  { int rcu = uploads_before_compute(h); if (rcu) return rcu; }
  if (!h->targets_built) { int rc = mi355ndt_batch_build_targets(h); if (rc) return rc; }
  const int B = h->n_pairs;
  const size_t tp = h->tgt_pitch;
  hipStream_t s = h->stream;
  std::vector<GridDesc> gd(B);
  HIPCHK(h, hipMemcpyAsync(gd.data(), h->d_grid, (size_t)B * sizeof(GridDesc), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  // which pairs go where: an empty target or source scores DBL_MAX with no launch, a grid -> k_fitness_batch, no grid -> k_fitness_brute_batch
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
    if (gd[b].status == GRID_EMPTY || ns <= 0) continue;   // (an empty source: DBL_MAX, 0 -- the single call refuses it, MI355NDT_ERR_STATE)
    nblk[b] = (ns + 255) / 256;
    part0[b] = n_part;
    n_part += nblk[b];
  }
  if (any_ok && !h->fit_index_ready) {
    HIPCHK(h, h->d_fwords.reserve(total_words));
    HIPCHK(h, h->d_fruns.reserve((size_t)B * (tp + 1)));
    HIPCHK(h, hipMemsetAsync(h->d_fwords, 0, total_words * sizeof(BitWord), s));
    const dim3 pg((unsigned)((tp + 255) / 256), (unsigned)B);
    k_fit_mark<<<pg, 256, 0, s>>>(h->d_keys_b, tp, h->d_grid, h->d_fwords, h->last_cb);
    k_fit_rank<<<B, 1024, 0, s>>>(h->d_grid, h->d_fwords);
    k_fit_runs<<<pg, 256, 0, s>>>(h->d_keys_b, tp, h->d_grid, h->d_fwords, h->d_fruns, h->last_cb);
    HIPCHK(h, hipGetLastError());
    h->fit_index_ready = true;
  }
  // item tables of the two launches: a grid -> k_fitness_batch, no grid -> k_fitness_brute_batch
  std::vector<int> tab, tab_brute;
  int gmax = 0, gmax_brute = 0;
  for (const bool with_grid : {true, false})
    fit_item_table(B, nblk, part0, [&](int b) { return (gd[b].status == GRID_OK) == with_grid; },
                   [&](int b) {
                     // rings needed to cover sqrt(max_range) (+1 cell of slack), as mi355ndt_fitness_score_T computes them
                     const double rr = with_grid ? std::sqrt(std::min(max_range, 1e30)) / (double)gd[b].leaf + 2.0 : 0.0;
                     return std::array<int, 3>{h->h_src_cnt[b], h->h_tgt_cnt[b], rr > (double)(1 << 30) ? (1 << 30) : (int)rr};
                   }, with_grid ? tab : tab_brute, with_grid ? gmax : gmax_brute);
  const size_t brute_at = tab.size();
  tab.insert(tab.end(), tab_brute.begin(), tab_brute.end());
  // transforms: the caller's, the final poses the last align left in d_results (read there, no host round trip), or the identity
  const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float* dT = nullptr;
  int Tstride = 16;
  if (n_part > 0) {
    static_assert(sizeof(mi355ndt_result) % sizeof(float) == 0 && offsetof(mi355ndt_result, final_colmajor) == 0, "final pose at the head of a result");
    if (T_colmajor) {
      HIPCHK(h, h->d_fit_T.reserve((size_t)B * 16));
      HIPCHK(h, hipMemcpyAsync(h->d_fit_T, T_colmajor, (size_t)B * 16 * sizeof(float), hipMemcpyHostToDevice, s));
      dT = h->d_fit_T;
    } else if (h->aligned_once) {
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
    static_assert(sizeof(FitItem) == 6 * sizeof(int), "FitItem is six ints");
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

// replaces calculateScore(cloud) (ndt_omp.h:232, ndt_omp_impl2.hpp:1006-1040)
int mi355ndt_calculate_score(mi355ndt_handle* h, const void* pts, size_t n, size_t stride, double* score) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!score || (!pts && n) || (n && stride < 12) || n >= (1u << 31)) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs != 1 || !h->have_target || h->h_tgt_cnt[0] <= 0) return MI355NDT_ERR_STATE;
  if (n == 0) { *score = std::nan(""); return MI355NDT_OK; }                     // 0 / 0 in the reference
  HIPCHK(h, hipSetDevice(h->device));
  { int rcu = uploads_before_compute(h); if (rcu) return rcu; }
  if (!h->targets_built || !h->cent_built || !h->icov64_built) {                // f32 centroids + f64 inverse covariances: the "live" build flavour
    const mi355ndt_params keep = h->prm;
    h->prm.step_size = 0; h->prm.trans_epsilon = 0;
    const int rc = mi355ndt_batch_build_targets(h);
    h->prm = keep;
    if (rc) return rc;
  }
  const size_t pitch = (n + 63) & ~(size_t)63;
  HIPCHK(h, h->d_score_pts.reserve(3 * pitch));
  const int blocks = (int)((n + SCORE_THREADS - 1) / SCORE_THREADS);
  HIPCHK(h, h->d_score_part.reserve((size_t)blocks));
  int rc = upload_cloud(h, h->d_score_pts, pitch, 0, pts, n, stride);
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
