// ndt_host_kffitness.hpp -- mi355ndt_keyframe_fitness_scores (graph edges between resident keyframes, ndt_kffitness.hpp) and the host
// arithmetic of InformationMatrixCalculator::calc_information_matrix (mi355ndt_information_matrix), and the build of a cloud's index, which
// the outlier removal and GICP call too.  The batch, the grids, the prefilter result, the keyframes' rows and the indexes that exist are left
// as they were; the index builds' sort and the call's tables use the shared scratch (h->vs).
#pragma once

// ---- a cloud's spatial index -------------------------------------------------------------------------
// one block: KfiHead (128 B) | BitWord words[nw] | unsigned runs[pitch + 1] (to 16 B) | float sorted[3][pitch] | unsigned ids[pitch]
struct KfiLayout { size_t words, runs, sorted, ids, bytes; int max_cells; };
static KfiLayout kfi_layout(size_t pitch) {
  KfiLayout L;
  L.max_cells = (int)std::min((size_t)KFI_MAX_CELLS, std::max((size_t)4096, 64 * pitch));   // at most 16 B of bitmap per point
  const size_t nw = (size_t)L.max_cells / 64 + 2;
  L.words = 128;
  L.runs = L.words + nw * sizeof(BitWord);
  L.sorted = L.runs + (((pitch + 1) * sizeof(unsigned) + 15) & ~(size_t)15);
  L.ids = L.sorted + 3 * pitch * sizeof(float);
  L.bytes = L.ids + pitch * sizeof(unsigned);
  return L;
}

// the index of a cloud as the kernels take it, with the cloud's own rows ([3][pitch], n points)
static KfiView kfi_view(const CloudIndex& ix, const float* rows, size_t pitch, size_t n) {
  const KfiLayout L = kfi_layout(pitch);
  const unsigned char* blob = ix.blob;
  return KfiView{reinterpret_cast<const GridDesc*>(blob), reinterpret_cast<const BitWord*>(blob + L.words), reinterpret_cast<const unsigned*>(blob + L.runs),
                 reinterpret_cast<const float*>(blob + L.sorted), reinterpret_cast<const unsigned*>(blob + L.ids), rows, (unsigned)pitch, (int)n};
}

// enqueue the build of `ix` over `n` points of SoA rows (n > 0), the lattice starting from cells of `cell_mm`; the lattice's status and the
// cloud's searchable points land in vs.stat[2 * slot] and [2 * slot + 1]: the caller fetches them with its results and hands them to
// kfi_built.  The scratch is sized by the caller (pitch; two status words per slot).  Every surface's index is built here.
static int kfi_build_rows(mi355ndt_handle* h, const float* rows, size_t pitch, size_t n, int cell_mm, CloudIndex& ix, int slot) {
  hipStream_t s = h->stream;
  const KfiLayout L = kfi_layout(pitch);
  ix.status = CloudIndex::NO_INDEX;
  HIPCHK(h, ix.blob.reserve(L.bytes));
  unsigned char* blob = ix.blob;
  KfiHead* head = reinterpret_cast<KfiHead*>(blob);
  GridDesc* gd = &head->gd;
  BitWord* words = reinterpret_cast<BitWord*>(blob + L.words);
  unsigned* runs = reinterpret_cast<unsigned*>(blob + L.runs);
  HIPCHK(h, hipMemsetAsync(blob, 0, L.runs, s));   // header and bitmap (k_kfi_gather adds into the one, k_fit_mark ORs into the other)
  const int gx = (int)((pitch + 255) / 256);
  const int cb = KFI_CELL_BITS;
  VoxelScratch& w = h->vs;
  unsigned* mm = reinterpret_cast<unsigned*>(w.mm.p);
  k_kfi_begin<<<1, 64, 0, s>>>(mm, w.cnt, (int)n);
  k_minmax<<<dim3(std::max(1, std::min((gx + 3) / 4 / MM_ILP, 64)), 1), 256, 0, s>>>(rows, pitch, w.cnt, mm);
  k_kfi_grid<<<1, 1, 0, s>>>(mm, (float)cell_mm * 1e-3f, L.max_cells, head, w.stat + 2 * slot);
  // stable sort by cell, the first pass computing the keys from the points (ndt_segsort.hpp); one segment
  const RsPoints points = {rows, w.cnt, gd, cb, w.keys};
  const RsSorted r = rs_sort_one_segment(s, cb, w.keys, w.vals, w.keys + pitch, w.vals + pitch, pitch, w.hist, w.offs, &points);
  const dim3 pg((unsigned)gx, 1u);
  k_fit_mark<<<pg, 256, 0, s>>>(r.keys, pitch, gd, words, cb);
  k_fit_rank<<<1, 1024, 0, s>>>(gd, words);
  k_fit_runs<<<pg, 256, 0, s>>>(r.keys, pitch, gd, words, runs, cb);
  k_kfi_gather<<<gx, 256, 0, s>>>(rows, pitch, (int)n, r.vals, reinterpret_cast<float*>(blob + L.sorted), reinterpret_cast<unsigned*>(blob + L.ids), head,
                                  w.stat + 2 * slot);
  HIPCHK(h, hipGetLastError());
  return MI355NDT_OK;
}
// ... and what the host learned of it: ret = the fetched vs.stat
static void kfi_built(CloudIndex& ix, const int* ret, int slot) { ix.status = ret[2 * slot]; ix.n_fin = ret[2 * slot + 1]; }

// replaces InformationMatrixCalculator::calc_fitness_score (information_matrix_calculator.cpp:53-87) for E graph edges at once
int mi355ndt_keyframe_fitness_scores(mi355ndt_handle* h, int n_edges, const int* ids1, const int* ids2, const double* relposes, double max_range,
                                     double* scores, long long* n_inliers) {
  using Keyframe = mi355ndt_handle::Keyframe;
  constexpr int NO_INDEX = CloudIndex::NO_INDEX;
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (n_edges < 0) return MI355NDT_ERR_BAD_ARG;
  if (n_edges == 0) return MI355NDT_OK;
  if (!ids1 || !ids2 || !relposes || !scores) return MI355NDT_ERR_BAD_ARG;
  const int E = n_edges;
  std::vector<Keyframe*> k1((size_t)E), k2((size_t)E);
  long long n_blocks = 0;
  for (int e = 0; e < E; e++) {
    k1[(size_t)e] = kf_find(h, ids1[e], "keyframe_fitness_scores");
    k2[(size_t)e] = k1[(size_t)e] ? kf_find(h, ids2[e], "keyframe_fitness_scores") : nullptr;
    if (!k2[(size_t)e]) return MI355NDT_ERR_BAD_ARG;
    n_blocks += (long long)((k2[(size_t)e]->n + 255) / 256);
  }
  if (n_blocks >= (1ll << 28)) { h->err = "keyframe_fitness_scores: too many points in all the edges of one call"; return MI355NDT_ERR_BAD_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = uploads_before_compute(h);             // (a keyframe_add's transfer may still be on its way)
  if (rc) return rc;
  hipStream_t s = h->stream;

  // the indexes this call needs and does not find: every searched keyframe once, however many edges name it.  (An empty side costs nothing.)
  std::map<Keyframe*, int> todo;
  size_t ws_pitch = 0;
  for (int e = 0; e < E; e++) {
    Keyframe* kf = k1[(size_t)e];
    if (kf->n == 0 || k2[(size_t)e]->n == 0 || kf->index.status != NO_INDEX || todo.count(kf)) continue;
    const int slot = (int)todo.size();
    todo.emplace(kf, slot);
    ws_pitch = std::max(ws_pitch, kf->pitch);
  }
  // which edges go where.  known[e]: the host has the status of the searched keyframe's index (built by an earlier call); an index built
  // by this call is in both tables and the kernels decide by its status -- the call waits for the device once, at its end
  const float mr = fit_range_f32(max_range);
  std::vector<int> part0((size_t)E, 0), nblk((size_t)E, 0), st((size_t)E, GRID_EMPTY);
  int n_part = 0;
  for (int e = 0; e < E; e++) {
    const Keyframe *a = k1[(size_t)e], *b = k2[(size_t)e];
    if (a->n == 0 || b->n == 0 || a->index.status == GRID_EMPTY) continue;   // DBL_MAX, 0 without a launch
    st[(size_t)e] = a->index.status;
    nblk[(size_t)e] = (int)((b->n + 255) / 256);
    part0[(size_t)e] = n_part;
    n_part += nblk[(size_t)e];
  }
  // item tables of the two launches: an edge whose searched keyframe has a lattice -> k_kf_fitness, none -> k_kf_fitness_brute, an index
  // this call builds -> both (the kernels decide by its status)
  std::vector<int> tab, tab_brute;
  int gmax = 0, gmax_brute = 0;
  for (const bool with_grid : {true, false})
    fit_item_table(E, nblk, part0, [&](int e) { return st[(size_t)e] == NO_INDEX || (st[(size_t)e] == GRID_OK) == with_grid; },
                   [&](int e) { return std::array<int, 3>{(int)k2[(size_t)e]->n, (int)k1[(size_t)e]->n, 0}; },
                   with_grid ? tab : tab_brute, with_grid ? gmax : gmax_brute);
  static_assert(sizeof(KfEdge) % 8 == 0, "the tables' layout");
  const size_t at_ok = (size_t)E * sizeof(KfEdge), at_brute = at_ok + tab.size() * sizeof(int), bytes = at_brute + tab_brute.size() * sizeof(int);
  VoxelScratch& w = h->vs;
  VsNeed need;
  need.pitch = ws_pitch; need.tab = n_part > 0 ? bytes : 0; need.part = (size_t)2 * n_part; need.stat = 2 * todo.size();
  rc = vs_reserve(h, need);
  if (rc) return rc;
  for (auto& t : todo) { rc = kfi_build_rows(h, t.first->rows, t.first->pitch, t.first->n, h->kff_cell_mm, t.first->index, t.second); if (rc) return rc; }
  if (n_part > 0) {
    unsigned char* ht = w.h_tab;
    KfEdge* he = reinterpret_cast<KfEdge*>(ht);
    for (int e = 0; e < E; e++) {
      const Keyframe *a = k1[(size_t)e], *b = k2[(size_t)e];
      KfEdge& x = he[e];
      memset(&x, 0, sizeof x);
      if (nblk[(size_t)e]) { x.src = b->rows; x.spitch = (unsigned)b->pitch; x.tgt = kfi_view(a->index, a->rows, a->pitch, a->n); }
      for (int k = 0; k < 16; k++) x.T[k] = (float)relposes[16 * (size_t)e + k];   // relpose.cast<float>() (:62)
    }
    memcpy(ht + at_ok, tab.data(), tab.size() * sizeof(int));
    memcpy(ht + at_brute, tab_brute.data(), tab_brute.size() * sizeof(int));
    w.pending = true;
    HIPCHK(h, hipMemcpyAsync(w.tab, ht, bytes, hipMemcpyHostToDevice, s));
    const unsigned char* dt = w.tab;
    const KfEdge* de = reinterpret_cast<const KfEdge*>(dt);
    const int* t_ok = reinterpret_cast<const int*>(dt + at_ok);
    const int* t_brute = reinterpret_cast<const int*>(dt + at_brute);
    if (gmax) k_kf_fitness<<<8u * (unsigned)gmax, 256, 0, s>>>(reinterpret_cast<const FitItem*>(t_ok + 16), t_ok, de, mr, max_range, w.part);
    if (gmax_brute) k_kf_fitness_brute<<<8u * (unsigned)gmax_brute, 256, 0, s>>>(reinterpret_cast<const FitItem*>(t_brute + 16), t_brute, de, mr, w.part);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(w.h_part, w.part, (size_t)2 * n_part * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (!todo.empty()) HIPCHK(h, hipMemcpyAsync(w.h_ret, w.stat, 2 * todo.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));             // the call's one wait
  w.pending = false;
  HIPCHK(h, hipGetLastError());
  for (auto& t : todo) kfi_built(t.first->index, w.h_ret, t.second);
  for (int e = 0; e < E; e++) fit_reduce(w.h_part + 2 * (size_t)part0[(size_t)e], nblk[(size_t)e], scores + e, n_inliers ? n_inliers + e : nullptr);
  return MI355NDT_OK;
}

// ---- the weighting half of calc_information_matrix: plain host arithmetic ------------------------------
void mi355ndt_inf_params_default(mi355ndt_inf_params* p) {
  if (!p) return;
  p->use_const_inf_matrix = 0;                    // information_matrix_calculator.cpp:11-20
  p->const_stddev_x = 0.5; p->const_stddev_q = 0.1;
  p->var_gain_a = 20.0;
  p->min_stddev_x = 0.1; p->max_stddev_x = 5.0;
  p->min_stddev_q = 0.05; p->max_stddev_q = 0.2;
  p->fitness_score_thresh = 0.5;
}

// information_matrix_calculator.hpp:40-44
static double inf_weight(double a, double max_x, double min_y, double max_y, double x) {
  const double y = (1.0 - std::exp(-a * x)) / (1.0 - std::exp(-a * max_x));
  return min_y + (max_y - min_y) * y;
}

int mi355ndt_information_matrix(const mi355ndt_inf_params* p, double fitness_score, double inf[36]) {
  if (!p || !inf) return MI355NDT_ERR_BAD_ARG;
  double dx, dq;
  if (p->use_const_inf_matrix) {                  // (:32-33: the stddev, not the variance)
    dx = p->const_stddev_x; dq = p->const_stddev_q;
  } else {
    const double min_var_x = std::pow(p->min_stddev_x, 2), max_var_x = std::pow(p->max_stddev_x, 2);
    const double min_var_q = std::pow(p->min_stddev_q, 2), max_var_q = std::pow(p->max_stddev_q, 2);
    const float w_x = (float)inf_weight(p->var_gain_a, p->fitness_score_thresh, min_var_x, max_var_x, fitness_score);   // (:44-45: a float)
    const float w_q = (float)inf_weight(p->var_gain_a, p->fitness_score_thresh, min_var_q, max_var_q, fitness_score);
    dx = (double)w_x; dq = (double)w_q;
  }
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      const double id = r == c ? 1.0 : 0.0;
      inf[6 * r + c] = (r < 3 && c < 3) ? id / dx : ((r >= 3 && c >= 3) ? id / dq : id);   // every entry of the two 3x3 blocks is divided
    }
  return MI355NDT_OK;
}
