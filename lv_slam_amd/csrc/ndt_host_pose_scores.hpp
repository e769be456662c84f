// ndt_host_pose_scores.hpp -- mi355ndt_batch_score_poses: many (pair, pose) scores of the bound batch in one copy of the call's tables, two
// launches and one wait (kernels: ndt_pose_scores.hpp).  The call owns its pose table, its row buffer and its landing block: the batch's pair
// states, results and partial rows are not touched, and nothing of the align workspace is re-sized.
#pragma once

using PoseScoreKernel = void (*) NDT_POSE_SCORE_ARGS_T;
static PoseScoreKernel pose_score_kernel(bool pca, int K, int ord) {
#define NDT_ROW(PCA, K_, ORD) if (pca == PCA && K == K_ && ord == ORD) return k_pose_scores<PCA, K_, ORD>;
  NDT_POSE_SCORE_ROWS(NDT_ROW)
#undef NDT_ROW
  return nullptr;
}

// the configurations the call does not serve (include/mi355_ndt.h), asked before anything else is looked at; null: served
static const char* pose_scores_refuses(const mi355ndt_handle* h) {
  if (h->ndt_class == NDT_CLASS_PCL) return "mi355ndt_batch_score_poses: not served under MI355NDT_OPT_NDT_CLASS = 1";
  if (h->pose_model == POSE_MODEL_EULER) return "mi355ndt_batch_score_poses: not served under MI355NDT_OPT_POSE_MODEL = 1";
  if (h->ground_class != GROUND_CLASS_NONE) return "mi355ndt_batch_score_poses: not served under a non-zero MI355NDT_OPT_GROUND_CLASS";
  if (h->arith != 0) return "mi355ndt_batch_score_poses: not served under MI355NDT_OPT_ARITH = 1 (its grids are tree-summed and its records are another layout)";
  if (is_pca_kd(h->prm)) return "mi355ndt_batch_score_poses: not served for ndt_pca + KDTREE (order-dependent weights, a kernel of its own)";
  return nullptr;
}

int mi355ndt_batch_score_poses(mi355ndt_handle* h, int n_items, const int* pairs, const float* poses_colmajor, double* scores, long long* hits) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (const char* why = pose_scores_refuses(h)) { h->err = why; return MI355NDT_ERR_UNSUPPORTED; }
  if (n_items < 0 || n_items > MI355NDT_SCORE_POSES_MAX_ITEMS) { h->err = "mi355ndt_batch_score_poses: n_items outside 0 .. MI355NDT_SCORE_POSES_MAX_ITEMS"; return MI355NDT_ERR_BAD_ARG; }
  if (n_items == 0) return MI355NDT_OK;
  if (!pairs || !poses_colmajor || !scores) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs <= 0 || !h->d_tgt || !h->d_src || !h->have_target || !h->have_source) return MI355NDT_ERR_STATE;
  const int B = h->n_pairs, n = n_items;
  for (int e = 0; e < n; e++) {
    if (pairs[e] < 0 || pairs[e] >= B) { h->err = "mi355ndt_batch_score_poses: item " + std::to_string(e) + " names pair " + std::to_string(pairs[e]) + ", outside the batch"; return MI355NDT_ERR_BAD_ARG; }
    for (int a = 0; a < 16; a++)
      if (!std::isfinite(poses_colmajor[(size_t)16 * e + a])) { h->err = "mi355ndt_batch_score_poses: the pose of item " + std::to_string(e) + " has a non-finite entry"; return MI355NDT_ERR_BAD_ARG; }
  }
  SweepConst sc;
  make_sweep_const(h, sc);
  const PoseScoreKernel kern = pose_score_kernel(sc.pca != 0, sc.K, h->f32_sum_order);
  if (!kern) { h->err = "mi355ndt_batch_score_poses: no kernel serves this configuration"; return MI355NDT_ERR_UNSUPPORTED; }
  // ---- nothing is refused from here on
  int rc = ensure_grids(h, GRIDS_CONFIG);          // (the engine's device, the uploads so far in front of the compute stream, the grids this configuration's sweeps read)
  if (rc) return rc;
  make_sweep_const(h, sc);                         // (the leaf size is the built grids')
  h->ev_last_fresh = false;
  // the items sorted by pair (stable: a pair's items keep the caller's order), one segment per pair that is named and has points
  auto& ps = h->pose_scores;
  std::vector<int> order((size_t)n), first((size_t)B + 1, 0);
  for (int e = 0; e < n; e++) first[(size_t)pairs[e] + 1]++;
  for (int b = 0; b < B; b++) first[(size_t)b + 1] += first[(size_t)b];
  { std::vector<int> at(first.begin(), first.end() - 1); for (int e = 0; e < n; e++) order[(size_t)at[(size_t)pairs[e]]++] = e; }
  std::vector<PoseSeg> segs;
  std::vector<PoseItem> items((size_t)n);
  long long work = 0, row_words = 0;
  for (int b = 0; b < B; b++) {
    const int cnt = first[(size_t)b + 1] - first[(size_t)b], np = h->h_src_cnt[(size_t)b];
    if (cnt == 0) continue;
    const int n_rows = ((np + CHUNK_PTS - 1) / CHUNK_PTS) * QUARTERS;       // batch-mode rows: four per chunk of the row tree
    for (int j = 0; j < cnt; j++) {
      // (the lacing of score-only rows: ndt_pose_scores.hpp)
      const long long row0 = row_words + (long long)(j / POSE_LACE) * (n_rows + 1) * NACC + 2 * (j % POSE_LACE);
      items[(size_t)order[(size_t)first[(size_t)b] + j]] = PoseItem{row0, b, np, b, n_rows};
    }
    row_words += (long long)((cnt + POSE_LACE - 1) / POSE_LACE) * (n_rows + 1) * NACC;
    if (n_rows == 0) continue;                     // an empty source: no work item, the row tree of no chunk is 0.0 / 0
    segs.push_back(PoseSeg{work, first[(size_t)b], cnt, n_rows, 0});
    work += (long long)cnt * n_rows;
  }
  // one block of tables: items, segments, poses (T's twelve words, row-major 3 x 4), order
  const size_t o_items = 0, o_segs = o_items + (size_t)n * sizeof(PoseItem), o_poses = o_segs + std::max<size_t>(segs.size(), 1) * sizeof(PoseSeg),
               o_order = o_poses + (size_t)n * POSE_WORDS * sizeof(float), bytes = o_order + (size_t)n * sizeof(int);
  static_assert(sizeof(PoseItem) % 8 == 0 && sizeof(PoseSeg) % 8 == 0 && (POSE_WORDS * sizeof(float)) % 8 == 0, "the tables keep their alignment in one block");
  HIPCHK(h, ps.h_tab.reserve(bytes));
  HIPCHK(h, ps.d_tab.reserve(bytes));
  HIPCHK(h, ps.d_rows.reserve((size_t)std::max(row_words, 1LL)));
  HIPCHK(h, ps.h_out.reserve((size_t)2 * n, hipHostMallocMapped));
  double* d_out = ps.h_out.dev();
  if (!d_out) { h->err = "mi355ndt_batch_score_poses: no device view of the landing block"; return MI355NDT_ERR_HIP; }
  unsigned char* t = ps.h_tab;                     // (the engine's stream is idle here: every entry point returns synchronised)
  memcpy(t + o_items, items.data(), (size_t)n * sizeof(PoseItem));
  if (!segs.empty()) memcpy(t + o_segs, segs.data(), segs.size() * sizeof(PoseSeg));
  float* tp = reinterpret_cast<float*>(t + o_poses);
  for (int e = 0; e < n; e++)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) tp[(size_t)e * POSE_WORDS + r * 4 + c] = poses_colmajor[(size_t)16 * e + c * 4 + r];
  memcpy(t + o_order, order.data(), (size_t)n * sizeof(int));
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(ps.d_tab, ps.h_tab, bytes, hipMemcpyHostToDevice, s));
  const unsigned char* d = ps.d_tab;
  const PoseItem* d_items = reinterpret_cast<const PoseItem*>(d + o_items);
  if (work > 0) {
    // resident waves deal the work among themselves; a small call launches no more workgroups than it has work for (a multiple of 8: one share per XCD)
    int per_cu = 0;                                // (what the registers AND the item's LDS allow)
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), SWEEP_THREADS, 0) != hipSuccess || per_cu < 1) {
      (void)hipGetLastError();
      per_cu = pose_score_wpe(sc.pca != 0, sc.K);
    }
    const long long slots = ((long long)h->n_cu * per_cu) & ~7LL;
    const long long want = 8 * ((work + 8 * WAVES - 1) / (8 * WAVES));
    const dim3 grid((unsigned)std::max(8LL, std::min(slots, want)));
    kern<<<grid, SWEEP_THREADS, 0, s>>>(h->d_src, h->src_pitch, h->d_grid, h->d_words, h->d_recs, h->d_cent, d_items, reinterpret_cast<const int*>(d + o_order),
                                        reinterpret_cast<const PoseSeg*>(d + o_segs), (int)segs.size(), work, reinterpret_cast<const float*>(d + o_poses), ps.d_rows, sc);
  }
  k_pose_score_rows<<<(unsigned)n, UPD_THREADS, 0, s>>>(d_items, ps.d_rows, d_out, reinterpret_cast<long long*>(d_out + n));
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(s));
  memcpy(scores, ps.h_out, (size_t)n * sizeof(double));
  if (hits) memcpy(hits, ps.h_out + n, (size_t)n * sizeof(long long));
  return MI355NDT_OK;
}
