// ndt_host_outlier.hpp -- mi355ndt_prefilter_outliers: PrefilteringNodelet::outlier_removal (prefiltering_nodelet.cpp:128, 150-161) over the
// resident prefilter result, in place (ndt_outlier.hpp).  The index (a CloudIndex, rebuilt by every call), dist[] and its pinned twin are this
// surface's own; the index build's sort, the flags, the scan and the compaction target use the shared scratch (h->vs).  The batch, the
// grids, the keyframes and their indexes, the map-cloud and window workspaces are left as they were.
// Below it, mi355ndt_batch_remove_outliers: the same stage over the clouds batch slots hold, K clouds per launch chain (ndt_outlier_batch.hpp).
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

// what both surfaces refuse of the parameters, each with its own name in front of the message
static int outlier_params_check(mi355ndt_handle* h, const mi355ndt_outlier_params& p, const char* who) {
  const char* bad = nullptr;
  if (p.method != MI355NDT_OUTLIER_STATISTICAL && p.method != MI355NDT_OUTLIER_RADIUS) bad = "unknown method";
  else if (p.mean_k < 1 || p.mean_k > OL_MAX_K) bad = "mean_k outside 1..64";
  else if (std::isnan(p.stddev_mul)) bad = "stddev_mul is NaN";
  else if (p.min_neighbors < 0 || p.min_neighbors > OL_MAX_K) bad = "min_neighbors outside 0..64";
  else if (!(p.radius >= 0.0)) bad = "radius is NaN or negative";
  if (!bad) return MI355NDT_OK;
  h->err = std::string(who) + ": " + bad;
  return MI355NDT_ERR_BAD_ARG;
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
  int rc = outlier_params_check(h, *p, "prefilter_outliers");
  if (rc) return rc;
  if (!h->d_pf_out) { h->err = "prefilter_outliers: no prefilter result is resident (mi355ndt_prefilter first)"; return MI355NDT_ERR_STATE; }
  const size_t ch = (size_t)h->pf_ch;               // (a result with an intensity row: compacted with the points, written out at the input's offset)
  if (ch == 4 && out_pts && (size_t)h->pf_ioff + 4 > out_stride) {
    h->err = "prefilter_outliers: the resident result carries an intensity at byte " + std::to_string(h->pf_ioff) + " of a record; out_stride_bytes " +
             std::to_string(out_stride) + " cannot hold it";
    return MI355NDT_ERR_BAD_ARG;
  }
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
  need.pitch = pitch; need.x = ch * pitch; need.stat = 2;
  rc = vs_reserve(h, need);
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
  HIPCHK(h, hipMemsetAsync(w.x, 0, ch * pitch * sizeof(float), s));
  if (ch == 4) k_ol_compact<true><<<gx, 256, 0, s>>>(rows, pitch, w.flag, w.pos, w.x);
  else k_ol_compact<false><<<gx, 256, 0, s>>>(rows, pitch, w.flag, w.pos, w.x);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(rows, w.x, ch * pitch * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIPCHK(h, hipMemcpyAsync(w.h_ret, w.pos + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(w.h_ret + 1, w.flag + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  const size_t m = (size_t)w.h_ret[0] + (size_t)w.h_ret[1];
  h->pf_count = (int)m;
  *n_out = m;
  return pf_result_records(h, m, out_pts, out_capacity, out_stride);
}

// ---- the same stage over the clouds batch slots hold, K clouds per launch chain (ndt_outlier_batch.hpp) ---------------------------------
// The scratch of a group of K clouds of segment pitch rp, per point: the staged rows 12 B + the index pools (points in cell order 12, ids 4, run
// starts 4, at most 16 of bitmap: kfi_layout) + dist 4 + two key and two id arrays (sort ping-pong) 16 + flag 4 + pos 4 + keep 1 + the sort's
// tile histograms and offsets 4: 81 B (85 with the staged intensity plane, when some slot of the call carries one).  Groups are cut as the
// batch prefilter cuts them, under the same budget.
#define OLB_POINT_BYTES 81

// where the pools of a group sit in the scratch's blob (vs.out), in bytes; [0, runs) is zeroed before every group
struct OlbLayout { size_t heads, gds, cnt, words, runs, sorted, ids, dist, bytes; unsigned nwc; };
static OlbLayout olb_layout(size_t K, size_t rp) {
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  OlbLayout L;
  L.nwc = (unsigned)((size_t)kfi_layout(rp).max_cells / 64 + 2);
  L.heads = 0;
  L.gds = up(L.heads + K * sizeof(KfiHead));
  L.cnt = up(L.gds + K * sizeof(GridDesc));
  L.words = up(L.cnt + K * sizeof(int));
  L.runs = up(L.words + K * (size_t)L.nwc * sizeof(BitWord));
  L.sorted = up(L.runs + K * (rp + 1) * sizeof(unsigned));
  L.ids = up(L.sorted + 3 * K * rp * sizeof(float));
  L.dist = up(L.ids + K * rp * sizeof(unsigned));
  L.bytes = up(L.dist + K * rp * sizeof(float));
  return L;
}

template <int CAP>
static void outlier_batch_knn_launch(hipStream_t s, unsigned gmax, const int* tab, const OlbCloud* clouds, int method, int K, float r2) {
  const FitItem* items = reinterpret_cast<const FitItem*>(tab + 16);
  k_olb_knn<CAP, true><<<8u * gmax, OL_LANES, 0, s>>>(items, tab, clouds, method, K, r2);
  k_olb_knn<CAP, false><<<8u * gmax, OL_LANES, 0, s>>>(items, tab, clouds, method, K, r2);   // (the clouds without a lattice, over the same table)
}

// kernels_ms (may be null): the time of the chain's kernels, HIP events around every group's chain, summed
static int batch_outliers_impl(mi355ndt_handle* h, int first_pair, int n, int sides, const mi355ndt_outlier_params* prm,
                               size_t* target_counts_out, size_t* source_counts_out, mi355ndt_outlier_stats* target_stats,
                               mi355ndt_outlier_stats* source_stats, double* kernels_ms) {
  // every argument before anything is enqueued: a refused call changes nothing
  const char* who = "batch_remove_outliers";
  if (n <= 0 || first_pair < 0 || first_pair + n > h->n_pairs) { h->err = std::string(who) + ": slots outside the batch"; return MI355NDT_ERR_BAD_ARG; }
  if (sides < 1 || sides > 3) { h->err = std::string(who) + ": sides outside 1..3"; return MI355NDT_ERR_BAD_ARG; }
  if (h->d_tgt != h->d_tgt_own || h->d_src != h->d_src_own) { h->err = std::string(who) + ": device buffers are bound"; return MI355NDT_ERR_BAD_ARG; }
  if (((sides & 2) && !h->have_target) || ((sides & 1) && !h->have_source)) { h->err = std::string(who) + ": a side that has never been given a cloud"; return MI355NDT_ERR_BAD_ARG; }
  mi355ndt_outlier_params p;
  if (prm) p = *prm; else (void)mi355ndt_outlier_params_default(&p);
  int rc = outlier_params_check(h, p, who);
  if (rc) return rc;
  const bool statistical = p.method == MI355NDT_OUTLIER_STATISTICAL;
  const int method = statistical ? OL_STATISTICAL : OL_RADIUS;
  const int Kn = statistical ? p.mean_k : p.min_neighbors;
  const float r2 = (float)(p.radius * p.radius);
  if (target_stats && (sides & 2)) memset(target_stats, 0, (size_t)n * sizeof *target_stats);
  if (source_stats && (sides & 1)) memset(source_stats, 0, (size_t)n * sizeof *source_stats);
  struct Cl { bool tgt; int pair; size_t n; };
  std::vector<Cl> cl;                                   // pair after pair, the target before the source; an empty slot stays empty: no work
  size_t maxn = 0;
  for (int k = 0; k < n; k++)
    for (const bool tgt : {true, false}) {
      if (!(sides & (tgt ? 2 : 1))) continue;
      const size_t c = (size_t)(tgt ? h->h_tgt_cnt : h->h_src_cnt)[(size_t)(first_pair + k)];
      size_t* out = tgt ? target_counts_out : source_counts_out;
      if (out) out[k] = c;
      if (c) { cl.push_back(Cl{tgt, first_pair + k, c}); maxn = std::max(maxn, c); }
    }
  if (kernels_ms) *kernels_ms = 0.0;
  const int n_cl = (int)cl.size();
  bool with_i = false;                                  // some cloud's slot carries its intensity: the plane is staged and compacted beside the rows
  for (const Cl& c : cl) with_i = with_i || slot_intensity_row(h, c.tgt, c.pair);
  if (n_cl) {
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t rp_all = (maxn + 63) & ~(size_t)63;
    const int group = pfb_group_size(h, OLB_POINT_BYTES + (with_i ? 4 : 0), rp_all, n_cl);
    // the groups: a group's segment pitch is its own largest count, and its k-NN table is made here, before anything is enqueued
    struct Grp { int g0, K; size_t rp; std::vector<int> tab; int gmax; };
    std::vector<Grp> groups;
    VsNeed need;
    for (int g0 = 0; g0 < n_cl; g0 += group) {
      Grp g;
      g.g0 = g0; g.K = std::min(group, n_cl - g0); g.gmax = 0;
      size_t gm = 0;
      for (int k = 0; k < g.K; k++) gm = std::max(gm, cl[(size_t)(g0 + k)].n);
      g.rp = (gm + 63) & ~(size_t)63;
      if (Kn > 0) {                                     // the k-NN launch's table: a cloud's blocks of OL_LANES queries on one XCD
        std::vector<int> nblk((size_t)g.K), part0((size_t)g.K, 0);
        long long blocks = 0;
        for (int k = 0; k < g.K; k++) { nblk[(size_t)k] = (int)((cl[(size_t)(g0 + k)].n + OL_LANES - 1) / OL_LANES); blocks += nblk[(size_t)k]; }
        if (blocks >= (1ll << 28)) { h->err = std::string(who) + ": too many points in one group"; return MI355NDT_ERR_BAD_ARG; }
        fit_item_table(g.K, nblk, part0, [](int) { return true; },
                       [&](int k) { return std::array<int, 3>{(int)cl[(size_t)(g0 + k)].n, (int)cl[(size_t)(g0 + k)].n, 0}; }, g.tab, g.gmax);
      }
      need.tab = std::max(need.tab, (((size_t)g.K * sizeof(PfbItem) + 15) & ~(size_t)15) + (size_t)g.K * sizeof(OlbCloud) + g.tab.size() * sizeof(int) +
                                    (with_i ? 8 + (size_t)g.K * sizeof(float*) : 0));
      groups.push_back(std::move(g));
    }
    // sized once, for `group` clouds of the call's largest count: no group needs more, and the sort's tiles are counted per cloud
    need.clouds = (size_t)group; need.pitch = (size_t)group * rp_all; need.x = (with_i ? 4 : 3) * need.pitch;
    need.out = (olb_layout((size_t)group, rp_all).bytes + 3) / 4;
    need.part = (size_t)OLB_STAT_DOUBLES * group; need.stat = OLB_RES_WORDS(group);
    rc = vs_reserve(h, need);
    if (rc) return rc;
    VoxelScratch& w = h->vs;
    HipEvent ev[2];
    if (kernels_ms) for (auto& e : ev) HIPCHK(h, e.create(hipEventDefault));
    rc = uploads_before_compute(h);                     // (a slot's upload may still be on its way)
    if (rc) return rc;
    const RsPlan plan = rs_plan(KFI_CELL_BITS);
    for (const Grp& g : groups) {
      const int K = g.K;
      const size_t rp = g.rp, seg = (size_t)K * rp;
      const int tiles = (int)((rp + RS_TILE - 1) / RS_TILE);
      const OlbLayout L = olb_layout((size_t)K, rp);
      if (w.pending) { HIPCHK(h, hipStreamSynchronize(s)); w.pending = false; }
      unsigned char* blob = reinterpret_cast<unsigned char*>((float*)w.out);
      KfiHead* heads = reinterpret_cast<KfiHead*>(blob + L.heads);
      GridDesc* gds = reinterpret_cast<GridDesc*>(blob + L.gds);
      int* cnt = reinterpret_cast<int*>(blob + L.cnt);
      BitWord* words = reinterpret_cast<BitWord*>(blob + L.words);
      unsigned* runs = reinterpret_cast<unsigned*>(blob + L.runs);
      float* sorted = reinterpret_cast<float*>(blob + L.sorted);
      unsigned* ids = reinterpret_cast<unsigned*>(blob + L.ids);
      float* dist = reinterpret_cast<float*>(blob + L.dist);
      float* X = w.x;
      // the tables: the clouds' slots, their views, the k-NN launch's items
      const size_t at_cl = (K * sizeof(PfbItem) + 15) & ~(size_t)15, at_tab = at_cl + (size_t)K * sizeof(OlbCloud);
      const size_t at_oi = (at_tab + g.tab.size() * sizeof(int) + 7) & ~(size_t)7, tab_bytes = at_oi + (with_i ? (size_t)K * sizeof(float*) : 0);
      static_assert(sizeof(OlbCloud) % 8 == 0, "the tables' layout");
      unsigned char* ht = w.h_tab;
      unsigned char* dt = w.tab;
      PfbItem* hit = reinterpret_cast<PfbItem*>(ht);
      OlbCloud* hcl = reinterpret_cast<OlbCloud*>(ht + at_cl);
      for (int k = 0; k < K; k++) {
        const Cl& c = cl[(size_t)(g.g0 + k)];
        const size_t dp = c.tgt ? h->tgt_pitch : h->src_pitch;
        hit[k] = PfbItem{(c.tgt ? h->d_tgt_own : h->d_src_own) + (size_t)c.pair * 3 * dp, (unsigned long long)dp, (int)c.n, g.g0 + k};
        hcl[k] = OlbCloud{KfiView{&heads[k].gd, words + (size_t)k * L.nwc, runs + (size_t)k * (rp + 1), sorted + (size_t)k * 3 * rp, ids + (size_t)k * rp,
                                  X + (size_t)k * 3 * rp, (unsigned)rp, (int)c.n},
                          dist + (size_t)k * rp, (int*)w.flag + (size_t)k * rp};
        if (with_i) reinterpret_cast<float**>(ht + at_oi)[k] = slot_intensity_row(h, c.tgt, c.pair);
      }
      const PfbInt pi = {with_i ? X + 3 * seg : nullptr, with_i ? reinterpret_cast<float* const*>(dt + at_oi) : nullptr};
      if (!g.tab.empty()) memcpy(ht + at_tab, g.tab.data(), g.tab.size() * sizeof(int));
      w.pending = true;
      HIPCHK(h, hipMemcpyAsync(dt, ht, tab_bytes, hipMemcpyHostToDevice, s));
      const PfbItem* items = reinterpret_cast<const PfbItem*>(dt);
      const OlbCloud* dcl = reinterpret_cast<const OlbCloud*>(dt + at_cl);
      const int* dtab = reinterpret_cast<const int*>(dt + at_tab);
      int* res = w.stat;
      int* stat = res + OLB_STAT_AT(K);
      if (kernels_ms) HIPCHK(h, hipEventRecord(ev[0], s));
      HIPCHK(h, hipMemsetAsync(dist, 0, seg * sizeof(float), s));
      HIPCHK(h, hipMemsetAsync(w.flag, 0, seg * sizeof(int), s));
      HIPCHK(h, hipMemsetAsync(blob, 0, L.runs, s));     // headers, descriptors, counts and bitmaps (k_fit_mark ORs into the last)
      k_olb_begin<<<(6 * K + 2 + 255) / 256, 256, 0, s>>>(reinterpret_cast<unsigned*>(w.mm.p), res, cnt, items, K);
      if (with_i) k_olb_stage<true><<<xcd_grid(tiles, K), 256, 0, s>>>(items, K, tiles, X, rp, pi);
      else k_olb_stage<false><<<xcd_grid(tiles, K), 256, 0, s>>>(items, K, tiles, X, rp, pi);
      if (Kn > 0) {
        // K indexes at once: extremes, the cell rule, the segmented sort whose first pass computes the keys from the points, mark, rank, runs, gather
        const int gx = (int)((rp + 255) / 256);
        k_minmax<<<dim3((unsigned)std::max(1, std::min((gx + 3) / 4 / MM_ILP, 64)), (unsigned)K), 256, 0, s>>>(X, rp, cnt, reinterpret_cast<unsigned*>(w.mm.p));
        k_olb_grid<<<(K + 63) / 64, 64, 0, s>>>(reinterpret_cast<unsigned*>(w.mm.p), (float)h->ol_cell_mm * 1e-3f, items, K, L.nwc, gds, heads, stat);
        const RsPoints points = {X, cnt, gds, KFI_CELL_BITS, w.keys};
        unsigned *ka = w.keys, *va = w.vals, *kb = w.keys + seg, *vb = w.vals + seg;
        if (!rs_disjoint(ka, va, kb, vb, seg)) { h->err = "outlier batch: the sort's two buffer pairs overlap"; return MI355NDT_ERR_STATE; }
        for (int ps = 0; ps < plan.passes; ps++) {
          rs_pass(s, plan.bits, ka, va, kb, vb, rp, ps * plan.bits, w.hist, w.offs, tiles, K, ps == 0, ps == 0 ? &points : nullptr);
          std::swap(ka, kb); std::swap(va, vb);
        }
        const dim3 pg((unsigned)gx, (unsigned)K);
        k_fit_mark<<<pg, 256, 0, s>>>(ka, rp, gds, words, KFI_CELL_BITS);
        k_fit_rank<<<K, 1024, 0, s>>>(gds, words);
        k_fit_runs<<<pg, 256, 0, s>>>(ka, rp, gds, words, runs, KFI_CELL_BITS);
        k_olb_gather<<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, cnt, va, sorted, ids, heads, stat, K, tiles);
        if (Kn <= 32) outlier_batch_knn_launch<32>(s, (unsigned)g.gmax, dtab, dcl, method, Kn, r2);
        else outlier_batch_knn_launch<64>(s, (unsigned)g.gmax, dtab, dcl, method, Kn, r2);
      } else {                                          // RADIUS with min_neighbors = 0: every searchable point is kept
        k_olb_finite<<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, items, K, tiles, w.flag);
      }
      if (statistical) {
        k_olb_stats<<<K, OLB_STATS_THREADS, 0, s>>>(dist, rp, items, stat, Kn, p.stddev_mul, w.part);
        k_olb_flag<<<xcd_grid(tiles, K), 256, 0, s>>>(dist, rp, items, w.part, K, tiles, w.flag);
      }
      k_pfb_scan_totals<<<xcd_grid(tiles, K), 1024, 0, s>>>(w.flag, rp, w.tmp, tiles, K);
      k_pfb_scan_offsets<<<K, 1024, 0, s>>>(w.tmp, tiles, items, K, res);
      k_pfb_scan_apply<<<xcd_grid(tiles, K), 1024, 0, s>>>(w.flag, rp, w.tmp, w.pos, tiles, K);
      if (with_i) k_olb_emit<true><<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, w.flag, w.pos, items, res, K, tiles, pi);
      else k_olb_emit<false><<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, w.flag, w.pos, items, res, K, tiles, pi);
      HIPCHK(h, hipGetLastError());
      if (kernels_ms) HIPCHK(h, hipEventRecord(ev[1], s));
      rc = compute_enqueued(h);                         // later uploads into these slots wait for the emit
      if (rc) return rc;
      // the group's one wait: K counts, K status pairs and, for STATISTICAL, K statistics
      int* ret = w.h_ret;
      HIPCHK(h, hipMemcpyAsync(ret, res, OLB_RES_WORDS(K) * sizeof(int), hipMemcpyDeviceToHost, s));
      if (statistical) HIPCHK(h, hipMemcpyAsync(w.h_part, w.part, (size_t)OLB_STAT_DOUBLES * K * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      w.pending = false;
      HIPCHK(h, hipGetLastError());
      if (kernels_ms) { float ms = 0.f; HIPCHK(h, hipEventElapsedTime(&ms, ev[0], ev[1])); *kernels_ms += ms; }
      for (int k = 0; k < K; k++) {
        const Cl& c = cl[(size_t)(g.g0 + k)];
        const size_t m = (size_t)ret[k];
        cloud_changed(h, c.tgt, c.pair, m, slot_intensity_row(h, c.tgt, c.pair) != nullptr);
        size_t* out = c.tgt ? target_counts_out : source_counts_out;
        if (out) out[c.pair - first_pair] = m;
        mi355ndt_outlier_stats* st = c.tgt ? target_stats : source_stats;
        if (statistical && st) {
          const long long nf = (long long)ret[OLB_STAT_AT(K) + 2 * k + 1];
          const double* d = (const double*)w.h_part + (size_t)OLB_STAT_DOUBLES * k;
          st[c.pair - first_pair] = mi355ndt_outlier_stats{(long long)c.n, nf >= (long long)Kn + 1 ? nf : 0, d[0], d[1], d[2]};
        }
      }
    }
  }
  return MI355NDT_OK;
}

int mi355ndt_batch_remove_outliers(mi355ndt_handle* h, int first_pair, int n, int sides, const mi355ndt_outlier_params* p,
                                   size_t* target_counts_out, size_t* source_counts_out,
                                   mi355ndt_outlier_stats* target_stats, mi355ndt_outlier_stats* source_stats) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  const int rc = batch_outliers_impl(h, first_pair, n, sides, p, target_counts_out, source_counts_out, target_stats, source_stats, nullptr);
  // an error exit may leave kernels queued that still use the scratch and the slot rows: later uploads wait for them all the same
  if (rc != MI355NDT_OK && rc != MI355NDT_ERR_BAD_ARG && h->ev_compute) (void)compute_enqueued(h);
  return rc;
}
