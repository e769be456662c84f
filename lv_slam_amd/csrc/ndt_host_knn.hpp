// ndt_host_knn.hpp -- mi355ndt_keyframe_knn / _knn_ids / _radius_search (ndt_knn.hpp): exact k-nearest and radius search over resident
// keyframes.  One body, knn_run: the items of a call -- (searched keyframe, query rows, pose) -- go through one launch chain and one wait;
// the host entry with queries of its own is the one-item case with the queries staged into the shared scratch (h->vs).  A searched
// keyframe's index is the keyframe's one CloudIndex: found, or built here by kfi_build_rows from MI355NDT_OPT_KF_FITNESS_CELL_MM and kept.
// The batch, the grids, the prefilter result and every keyframe's rows are left as they were.
#pragma once

int mi355ndt_knn_params_default(mi355ndt_knn_params* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  p->k = 1; p->max_range = INFINITY; p->query_order = MI355NDT_KNN_ORDER_AUTO;
  return MI355NDT_OK;
}

// What MI355NDT_KNN_ORDER_AUTO runs, as measured (tools/keyframe_knn_timing.py, DESIGN.md section 8: 65,536 queries against a 101 k point
// window keyframe).  Queries from the host: cell order gains 20-24 % (k = 5, 20) when they arrive in no order and costs the sort, 0.05 ms,
// when they happen to be in cell order already -- the two meet near 4,096 queries, below which the input order runs.  Queries that are a
// resident keyframe: a window keyframe's points leave the VoxelGrid in cell order, the sort gained nothing and cost 0.05 ms per item, and
// a call of many items would run one sort each: input order.
#define KNN_AUTO_CELL_MIN 4096
static bool knn_cell_order(int query_order, bool host_queries, size_t n) {
  return query_order == MI355NDT_KNN_ORDER_CELL || (query_order == MI355NDT_KNN_ORDER_AUTO && host_queries && n >= KNN_AUTO_CELL_MIN);
}

template <int CAP>
static void knn_launch(hipStream_t s, int gmax, int gmax_brute, const int* t_ok, const int* t_brute, const KnnItem* items, const KnnCall& c) {
  if (gmax) k_kf_knn<CAP, true><<<8u * (unsigned)gmax, OL_LANES, 0, s>>>(reinterpret_cast<const FitItem*>(t_ok + 16), t_ok, items, c);
  if (gmax_brute) k_kf_knn<CAP, false><<<8u * (unsigned)gmax_brute, OL_LANES, 0, s>>>(reinterpret_cast<const FitItem*>(t_brute + 16), t_brute, items, c);
}

// E items: keyframe kt[e] searched by the nq[e] queries of keyframe kq[e] -- or, kq == nullptr (E == 1), by the n host records at `pts` --
// moved by T[16 e ..] (column-major f32).  The results land concatenated in item order: ids / d2 [sum nq][K], counts [sum nq].
static int knn_run(mi355ndt_handle* h, int E, mi355ndt_handle::Keyframe* const* kt, mi355ndt_handle::Keyframe* const* kq, const void* pts, size_t n_host,
                   size_t stride, const float* T, const KnnCall& call, int query_order, int* ids, float* d2, int* counts) {
  using Keyframe = mi355ndt_handle::Keyframe;
  constexpr int NO_INDEX = CloudIndex::NO_INDEX;
  const bool cell = knn_cell_order(query_order, kq == nullptr, n_host);
  const size_t K = (size_t)call.K;
  std::vector<size_t> nq((size_t)E), off((size_t)E), poff((size_t)E);
  size_t N = 0, P = 0;
  long long n_blocks = 0;
  for (int e = 0; e < E; e++) {
    nq[(size_t)e] = kq ? kq[e]->n : n_host;
    off[(size_t)e] = N; poff[(size_t)e] = P;
    N += nq[(size_t)e]; P += (nq[(size_t)e] + 63) & ~(size_t)63;
    n_blocks += (long long)((nq[(size_t)e] + 63) / 64);
  }
  if (N == 0) return MI355NDT_OK;
  if (n_blocks >= (1ll << 28) || N * K >= ((size_t)1 << 31)) { h->err = "keyframe_knn: too many queries in all the items of one call"; return MI355NDT_ERR_BAD_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  int rc = uploads_before_compute(h);             // (a keyframe_add's transfer may still be on its way)
  if (rc) return rc;
  hipStream_t s = h->stream;

  // the indexes this call needs and does not find: every searched keyframe once, however many items name it
  std::map<Keyframe*, int> todo;
  size_t ws_pitch = 0;
  for (int e = 0; e < E; e++) {
    Keyframe* kf = kt[e];
    if (kf->n == 0 || nq[(size_t)e] == 0 || kf->index.status != NO_INDEX || todo.count(kf)) continue;
    const int slot = (int)todo.size();
    todo.emplace(kf, slot);
    ws_pitch = std::max(ws_pitch, kf->pitch);
  }
  // item tables of the two launches: a searched keyframe with a lattice -> the ring walk, without one or with nothing to search -> the
  // exhaustive variant, an index this call builds -> both (the kernels decide by its status)
  std::vector<int> nblk((size_t)E), part0((size_t)E, 0), st((size_t)E);
  for (int e = 0; e < E; e++) {
    nblk[(size_t)e] = (int)((nq[(size_t)e] + 63) / 64);
    st[(size_t)e] = kt[e]->n == 0 ? GRID_EMPTY : kt[e]->index.status;
  }
  std::vector<int> tab, tab_brute;
  int gmax = 0, gmax_brute = 0;
  for (const bool with_grid : {true, false})
    fit_item_table(E, nblk, part0, [&](int e) { return st[(size_t)e] == NO_INDEX || (st[(size_t)e] == GRID_OK) == with_grid; },
                   [&](int e) { return std::array<int, 3>{(int)nq[(size_t)e], (int)kt[e]->n, 0}; },
                   with_grid ? tab : tab_brute, with_grid ? gmax : gmax_brute);
  static_assert(sizeof(KnnItem) % 8 == 0, "the tables' layout");
  const size_t at_ok = (size_t)E * sizeof(KnnItem), at_brute = at_ok + tab.size() * sizeof(int), bytes = at_brute + tab_brute.size() * sizeof(int);
  const size_t qp = (n_host + 63) & ~(size_t)63;  // the staged host queries' pitch
  VoxelScratch& w = h->vs;
  VsNeed need;
  need.pitch = std::max(ws_pitch, cell ? P : (size_t)0);
  need.in = kq ? 0 : 3 * qp; need.x = cell ? 3 * P : 0; need.out = (2 * K + 1) * N;
  need.tab = bytes; need.stat = 2 * todo.size();
  rc = vs_reserve(h, need);
  if (rc) return rc;
  if (!kq) {                                      // the host queries, through the engine's staging into rows of the scratch
    const UpItem up = {w.in, qp, 0, pts, n_host, stride};
    rc = upload_items(h, &up, 1);
    if (!rc) rc = uploads_before_compute(h);
    if (rc) return rc;
  }
  for (auto& t : todo) { rc = kfi_build_rows(h, t.first->rows, t.first->pitch, t.first->n, h->kff_cell_mm, t.first->index, t.second); if (rc) return rc; }

  // results in the scratch: ids [N][K] | d2 [N][K] | counts [N]
  int* d_ids = reinterpret_cast<int*>(w.out.p);
  float* d_d2 = w.out.p + N * K;
  int* d_cnt = reinterpret_cast<int*>(w.out.p + 2 * N * K);
  // (the sort of KFI_CELL_BITS bits hops between the two halves of keys / vals: where an even number of passes ends)
  const bool back = rs_plan(KFI_CELL_BITS).passes % 2 == 0;
  unsigned char* ht = w.h_tab;
  KnnItem* he = reinterpret_cast<KnnItem*>(ht);
  for (int e = 0; e < E; e++) {
    const Keyframe* a = kt[e];
    KnnItem& x = he[e];
    memset(&x, 0, sizeof x);
    x.nq = (int)nq[(size_t)e];
    x.empty = a->n == 0 ? 1 : 0;
    if (kq) { x.q = kq[e]->rows; x.qpitch = (unsigned)kq[e]->pitch; } else { x.q = w.in; x.qpitch = (unsigned)qp; }
    if (!x.empty) x.tgt = kfi_view(a->index, a->rows, a->pitch, a->n);
    if (cell) { x.mq = w.x.p + poff[(size_t)e]; x.mpitch = (unsigned)P; x.poff = (unsigned)poff[(size_t)e]; x.order = w.vals.p + (back ? 0 : P) + poff[(size_t)e]; }
    x.ids = d_ids + off[(size_t)e] * K; x.d2 = d_d2 + off[(size_t)e] * K; x.counts = d_cnt + off[(size_t)e];
    memcpy(x.T, T + 16 * (size_t)e, sizeof x.T);
  }
  memcpy(ht + at_ok, tab.data(), tab.size() * sizeof(int));
  memcpy(ht + at_brute, tab_brute.data(), tab_brute.size() * sizeof(int));
  w.pending = true;
  HIPCHK(h, hipMemcpyAsync(w.tab, ht, bytes, hipMemcpyHostToDevice, s));
  const unsigned char* dt = w.tab;
  const KnnItem* de = reinterpret_cast<const KnnItem*>(dt);
  const int* t_ok = reinterpret_cast<const int*>(dt + at_ok);
  const int* t_brute = reinterpret_cast<const int*>(dt + at_brute);
  if (cell) {                                     // moved rows and keys of every item, then one stable sort per item
    size_t pmax = 0;
    for (int e = 0; e < E; e++) pmax = std::max(pmax, (nq[(size_t)e] + 63) & ~(size_t)63);
    for (int e0 = 0; e0 < E; e0 += MAX_PAIRS) {
      const int cnt = std::min(E - e0, MAX_PAIRS);
      k_knn_keys<<<dim3((unsigned)((pmax + 255) / 256), (unsigned)cnt), 256, 0, s>>>(de + e0, w.keys, w.vals);
    }
    for (int e = 0; e < E; e++) {
      const size_t pe = (nq[(size_t)e] + 63) & ~(size_t)63, po = poff[(size_t)e];
      if (pe) (void)rs_sort_one_segment(s, KFI_CELL_BITS, w.keys + po, w.vals + po, w.keys + P + po, w.vals + P + po, pe, w.hist, w.offs);
    }
  }
  if (K <= 8) knn_launch<8>(s, gmax, gmax_brute, t_ok, t_brute, de, call);
  else if (K <= 32) knn_launch<32>(s, gmax, gmax_brute, t_ok, t_brute, de, call);
  else knn_launch<64>(s, gmax, gmax_brute, t_ok, t_brute, de, call);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(ids, d_ids, N * K * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(d2, d_d2, N * K * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(counts, d_cnt, N * sizeof(int), hipMemcpyDeviceToHost, s));
  if (!todo.empty()) HIPCHK(h, hipMemcpyAsync(w.h_ret, w.stat, 2 * todo.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));             // the call's one wait
  w.pending = false;
  HIPCHK(h, hipGetLastError());
  for (auto& t : todo) kfi_built(t.first->index, w.h_ret, t.second);
  return MI355NDT_OK;
}

// the call's constants; false with a message where an argument is refused
static bool knn_call_of(mi355ndt_handle* h, const char* where, int mode, int K, double range, KnnCall* c) {
  if (K < 1 || K > OL_MAX_K) { h->err = std::string(where) + (mode == KNN_MODE_RADIUS ? ": max_nn" : ": k") + " must be 1 .. 64"; return false; }
  if (!(range >= 0.0)) { h->err = std::string(where) + (mode == KNN_MODE_RADIUS ? ": the radius" : ": max_range") + " must be a number >= 0"; return false; }
  c->mode = mode; c->K = K;
  c->thr2 = range * range;
  c->bound = (float)c->thr2;
  if (mode == KNN_MODE_KNN && (double)c->bound <= c->thr2) c->bound = nextafterf(c->bound, INFINITY);   // the f32 just above the limit (icp_make_step)
  return true;
}
static bool knn_order_ok(mi355ndt_handle* h, const char* where, int query_order) {
  if (query_order == MI355NDT_KNN_ORDER_AUTO || query_order == MI355NDT_KNN_ORDER_INPUT || query_order == MI355NDT_KNN_ORDER_CELL) return true;
  h->err = std::string(where) + ": query_order must be 0 (the engine's choice), 1 (input order) or 2 (cell order)";
  return false;
}

static const float KNN_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// the two entries with host queries
static int knn_host(mi355ndt_handle* h, const char* where, int kf_id, const void* queries, size_t n, size_t stride, const float* T_colmajor, int mode, int K,
                    double range, int query_order, int* ids, float* d2, int* counts) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  KnnCall c;
  if (!knn_call_of(h, where, mode, K, range, &c) || !knn_order_ok(h, where, query_order)) return MI355NDT_ERR_BAD_ARG;
  mi355ndt_handle::Keyframe* kf = kf_find(h, kf_id, where);
  if (!kf) return MI355NDT_ERR_BAD_ARG;
  if (n == 0) return MI355NDT_OK;
  if (!queries || stride < 12) { h->err = std::string(where) + ": the queries are records of at least 12 bytes (x, y, z f32 first)"; return MI355NDT_ERR_BAD_ARG; }
  if (!ids || !d2 || !counts) { h->err = std::string(where) + ": ids, d2 and counts are all written: none may be NULL"; return MI355NDT_ERR_BAD_ARG; }
  if (n >= (1u << 30)) { h->err = std::string(where) + ": too many queries"; return MI355NDT_ERR_BAD_ARG; }
  return knn_run(h, 1, &kf, nullptr, queries, n, stride, T_colmajor ? T_colmajor : KNN_IDENTITY, c, query_order, ids, d2, counts);
}

int mi355ndt_keyframe_knn(mi355ndt_handle* h, int kf_id, const void* queries, size_t n, size_t stride_bytes, const float* T_colmajor,
                          const mi355ndt_knn_params* p, int* ids, float* d2, int* counts) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!p) return MI355NDT_ERR_BAD_ARG;
  return knn_host(h, "keyframe_knn", kf_id, queries, n, stride_bytes, T_colmajor, KNN_MODE_KNN, p->k, p->max_range, p->query_order, ids, d2, counts);
}

int mi355ndt_keyframe_radius_search(mi355ndt_handle* h, int kf_id, const void* queries, size_t n, size_t stride_bytes, const float* T_colmajor,
                                    double radius, int max_nn, int query_order, int* ids, float* d2, int* counts) {
  return knn_host(h, "keyframe_radius_search", kf_id, queries, n, stride_bytes, T_colmajor, KNN_MODE_RADIUS, max_nn, radius, query_order, ids, d2, counts);
}

int mi355ndt_keyframe_knn_ids(mi355ndt_handle* h, int n_items, const int* searched_ids, const int* query_ids, const double* relposes,
                              const mi355ndt_knn_params* p, size_t total_queries, int* ids, float* d2, int* counts) {
  using Keyframe = mi355ndt_handle::Keyframe;
  const char* where = "keyframe_knn_ids";
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!p || n_items < 0) return MI355NDT_ERR_BAD_ARG;
  KnnCall c;
  if (!knn_call_of(h, where, KNN_MODE_KNN, p->k, p->max_range, &c) || !knn_order_ok(h, where, p->query_order)) return MI355NDT_ERR_BAD_ARG;
  if (n_items == 0) return MI355NDT_OK;
  if (!searched_ids || !query_ids || !relposes) { h->err = std::string(where) + ": searched_ids, query_ids and relposes may not be NULL"; return MI355NDT_ERR_BAD_ARG; }
  const int E = n_items;
  std::vector<Keyframe*> kt((size_t)E), kq((size_t)E);
  size_t N = 0;
  for (int e = 0; e < E; e++) {
    kt[(size_t)e] = kf_find(h, searched_ids[e], where);
    kq[(size_t)e] = kt[(size_t)e] ? kf_find(h, query_ids[e], where) : nullptr;
    if (!kq[(size_t)e]) return MI355NDT_ERR_BAD_ARG;
    N += kq[(size_t)e]->n;
  }
  if (N != total_queries) {
    h->err = std::string(where) + ": total_queries is " + std::to_string(total_queries) + ", the query keyframes hold " + std::to_string(N) + " points";
    return MI355NDT_ERR_BAD_ARG;
  }
  if (N == 0) return MI355NDT_OK;
  if (!ids || !d2 || !counts) { h->err = std::string(where) + ": ids, d2 and counts are all written: none may be NULL"; return MI355NDT_ERR_BAD_ARG; }
  std::vector<float> T((size_t)16 * E);
  for (size_t k = 0; k < T.size(); k++) T[k] = (float)relposes[k];   // relpose.cast<float>(), as mi355ndt_keyframe_fitness_scores casts them
  return knn_run(h, E, kt.data(), kq.data(), nullptr, 0, 0, T.data(), c, p->query_order, ids, d2, counts);
}
