// ndt_host_gicp_batch.hpp -- mi355ndt_gicp_batch_*: every GICP candidate of one loop check against the surface's target, aligned in one
// lockstep batch (the loop detector's per-candidate loop, loop_detector.hpp:148-205, :211-281).  Each slot runs the single-pair outer loop
// and BFGS driver (gicp_outer, ndt_host_gicp.hpp) on a worker thread of its own; where that loop evaluates on the device the worker posts a
// request -- (match, G, T) or (cost, x, base), already turned into the kernel's GcMatch / GcCost by host arithmetic -- and blocks
// (gicp_lockstep.hpp).  The calling thread serves all posted requests with ONE round: a copy of the slot table, k_gc_match_batch,
// k_gc_cost_batch, k_gc_cost_final_batch, one wait (ndt_gicp.hpp, 4).  Workers never call HIP and never touch the handle; only the calling
// thread does.  The kernels' bodies and the host loop are the single-pair surface's, so every slot's result is that surface's, byte for byte.
// The single-pair surface (its clouds, correspondences, final transformation), the NDT batch, the grids and the keyframes' rows are left
// as they were; a keyframe's index and covariance cache are used, and filled, as that surface would.
#pragma once

typedef mi355ndt_handle::GicpBatch::Slot GicpBatchSlot;

static int gicp_batch_slot(mi355ndt_handle* h, const char* where, int slot, GicpBatchSlot** out) {
  auto& gb = h->gicp_batch;
  if (gb.slot.empty()) { h->err = std::string(where) + ": no slots are reserved (mi355ndt_gicp_batch_reserve first)"; return MI355NDT_ERR_STATE; }
  if (slot < 0 || slot >= (int)gb.slot.size()) {
    h->err = std::string(where) + ": slot " + std::to_string(slot) + " outside 0.." + std::to_string(gb.slot.size() - 1);
    return MI355NDT_ERR_BAD_ARG;
  }
  *out = &gb.slot[(size_t)slot];
  return MI355NDT_OK;
}

int mi355ndt_gicp_batch_reserve(mi355ndt_handle* h, int n_slots) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (n_slots < 1 || n_slots > MI355NDT_GICP_BATCH_MAX) {
    h->err = "gicp_batch_reserve: n_slots outside 1.." + std::to_string(MI355NDT_GICP_BATCH_MAX);
    return MI355NDT_ERR_BAD_ARG;
  }
  auto& gb = h->gicp_batch;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));     // nothing enqueued may still read what the earlier slots own
  gb.slot.clear();
  gb.rounds = 0; gb.requests.assign((size_t)n_slots, 0);
  HIPCHK(h, gb.m.reserve(MI355NDT_GICP_BATCH_MAX));
  HIPCHK(h, gb.d_tab.reserve(MI355NDT_GICP_BATCH_MAX));
  HIPCHK(h, gb.h_tab.reserve(MI355NDT_GICP_BATCH_MAX));
  if (!gb.h_rec) {
    HIPCHK(h, gb.h_rec.reserve((size_t)MI355NDT_GICP_BATCH_MAX * GC_REC, hipHostMallocMapped));
    gb.d_rec = gb.h_rec.dev();
    if (!gb.d_rec) { gb.h_rec = PinBuf<double>(); h->err = "gicp_batch_reserve: no device view of the mapped result records"; return MI355NDT_ERR_HIP; }
  }
  gb.slot.resize((size_t)n_slots);
  return MI355NDT_OK;
}

int mi355ndt_gicp_batch_set_source(mi355ndt_handle* h, int slot, const void* pts, size_t n, size_t stride_bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  GicpBatchSlot* sl;
  int rc = gicp_batch_slot(h, "gicp_batch_set_source", slot, &sl);
  if (rc) return rc;
  sl->have_final = false;
  return gicp_side_set_host(h, sl->side, pts, n, stride_bytes);
}

int mi355ndt_gicp_batch_set_source_keyframe(mi355ndt_handle* h, int slot, int id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  GicpBatchSlot* sl;
  int rc = gicp_batch_slot(h, "gicp_batch_set_source_keyframe", slot, &sl);
  if (rc) return rc;
  if (!kf_find(h, id, "gicp_batch_set_source_keyframe")) return MI355NDT_ERR_BAD_ARG;
  sl->side.kf_id = id; sl->side.set = true;
  sl->have_final = false;
  return MI355NDT_OK;
}

// ---- the lockstep round ----------------------------------------------------------------------------------
struct GicpBatchReq { int kind; GcMatch match; GcCost cost; };   // kind: 0 = a matching pass, 1 = a cost evaluation
struct GicpBatchRec { double v[GC_REC]; };                        // the slot's record: 13 sums, m
typedef gicp_lockstep::Lockstep<GicpBatchReq, GicpBatchRec> GicpSteps;

// a slot's evaluator (worker thread): host arithmetic, then the post; nothing of HIP, nothing of the handle
struct GicpEvalPosted {
  GicpSteps* ls; int k; const mi355ndt_gicp_params* prm;
  int match(const float* G, const float* T, int* m) {
    GicpBatchReq r{};
    GicpBatchRec o;
    r.kind = 0; r.match = gicp_make_match(*prm, G, T);
    const bool ok = ls->post(k, r, &o);
    *m = (int)o.v[GC_SUMS];
    return ok ? MI355NDT_OK : MI355NDT_ERR_HIP;
  }
  int sums(const double* x, const float* base, double* sums) {
    GicpBatchReq r{};
    GicpBatchRec o;
    r.kind = 1; r.cost = gicp_make_cost(x, base);
    const bool ok = ls->post(k, r, &o);
    for (int i = 0; i < GC_SUMS; i++) sums[i] = o.v[i];
    return ok ? MI355NDT_OK : MI355NDT_ERR_HIP;
  }
};

// one round on the calling thread: the table (matching passes first), at most three launches, one wait; m_last: each slot's matches
static int gicp_batch_round(mi355ndt_handle* h, const GicpView& D, const std::vector<GicpView>& S, const int* slots, int n,
                            const GicpBatchReq* req, GicpBatchRec* rec, std::vector<int>& m_last) {
  auto& gb = h->gicp_batch;
  hipStream_t s = h->stream;
  GcSlot* tab = gb.h_tab;
  int ne = 0, n_match = 0, chunks[2] = {0, 0};
  for (int kind = 0; kind < 2; kind++) {
    for (int j = 0; j < n; j++) {
      const int k = slots[j];
      if (req[k].kind != kind) continue;
      const GicpView& v = S[(size_t)k];
      GicpBatchSlot& sl = gb.slot[(size_t)k];
      GcSlot& e = tab[ne++];
      e.src = v.rows; e.c1 = v.cache->cov;
      e.idx = sl.idx; e.maha = sl.maha; e.m = gb.m + k; e.part = sl.part;
      e.rec = gb.d_rec + (size_t)k * GC_REC;
      e.spitch = (unsigned)v.pitch; e.n = (int)v.n;
      e.n_chunks = (int)((v.n + GC_CHUNK - 1) / GC_CHUNK);
      e.chunk0 = chunks[kind]; chunks[kind] += e.n_chunks;
      e.m_host = m_last[(size_t)k]; e.pad = 0;
      if (kind == 0) e.match = req[k].match; else e.cost = req[k].cost;
    }
    if (kind == 0) n_match = ne;
  }
  HIPCHK(h, hipMemcpyAsync(gb.d_tab, tab, (size_t)ne * sizeof(GcSlot), hipMemcpyHostToDevice, s));
  if (n_match) k_gc_match_batch<<<(unsigned)chunks[0], 256, 0, s>>>(gb.d_tab, n_match, kfi_view(*D.index, D.rows, D.pitch, D.n), D.cache->cov);
  if (ne > n_match) k_gc_cost_batch<<<(unsigned)chunks[1], GC_CHUNK, 0, s>>>(gb.d_tab + n_match, ne - n_match, D.rows, D.pitch);
  k_gc_cost_final_batch<<<(unsigned)ne, 256, 0, s>>>(gb.d_tab, n_match);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(s));
  for (int j = 0; j < n; j++) {
    const int k = slots[j];
    for (int i = 0; i < GC_REC; i++) rec[k].v[i] = gb.h_rec[(size_t)k * GC_REC + i];
    if (req[k].kind == 0) m_last[(size_t)k] = (int)rec[k].v[GC_SUMS];
  }
  return MI355NDT_OK;
}

int mi355ndt_gicp_batch_align(mi355ndt_handle* h, const float* guesses_colmajor, mi355ndt_gicp_result* results) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!guesses_colmajor || !results) return MI355NDT_ERR_BAD_ARG;
  auto& gb = h->gicp_batch;
  const int K = (int)gb.slot.size();
  if (!K) { h->err = "gicp_batch_align: no slots are reserved (mi355ndt_gicp_batch_reserve first)"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  GicpView D;
  std::vector<GicpView> S((size_t)K);
  std::vector<std::string> where((size_t)K);
  int rc = gicp_view(h, MI355NDT_GICP_TARGET, "gicp_batch_align", &D);
  for (int k = 0; k < K && !rc; k++) {
    where[(size_t)k] = "gicp_batch_align: slot " + std::to_string(k);
    rc = gicp_view_side(h, gb.slot[(size_t)k].side, where[(size_t)k].c_str(), " is unset", &S[(size_t)k]);
  }
  if (!rc) rc = gicp_prepare(h, "gicp_batch_align", D);
  for (int k = 0; k < K && !rc; k++) rc = gicp_prepare(h, where[(size_t)k].c_str(), S[(size_t)k]);
  if (rc) return rc;
  for (int k = 0; k < K; k++) {
    GicpBatchSlot& sl = gb.slot[(size_t)k];
    const GicpView& v = S[(size_t)k];
    HIPCHK(h, sl.idx.reserve(v.pitch)); HIPCHK(h, sl.maha.reserve(9 * v.pitch));
    HIPCHK(h, sl.part.reserve((v.n + GC_CHUNK - 1) / GC_CHUNK * GC_SUMS));
    sl.have_final = false;
  }
  HIPCHK(h, hipMemsetAsync(gb.m, 0, MI355NDT_GICP_BATCH_MAX * sizeof(int), h->stream));   // (a failed round may have left a count behind)

  const mi355ndt_gicp_params prm = h->gicp.prm;   // the workers' copy
  std::vector<mi355ndt_gicp_result> res((size_t)K);
  std::vector<std::array<float, 16>> fin((size_t)K);
  std::vector<int> rcs((size_t)K, MI355NDT_OK), m_last((size_t)K, 0);
  int round_rc = MI355NDT_OK;
  GicpSteps ls(K);
  const bool ok = ls.run(
      [&ls, &prm, &res, &fin, &rcs, guesses_colmajor](int k) {
        GicpEvalPosted ev{&ls, k, &prm};
        rcs[(size_t)k] = gicp_outer(ev, prm, guesses_colmajor + 16 * (size_t)k, fin[(size_t)k].data(), &res[(size_t)k]);
      },
      [&](const int* slots, int n, const GicpBatchReq* req, GicpBatchRec* rec) {
        round_rc = gicp_batch_round(h, D, S, slots, n, req, rec, m_last);
        return round_rc == MI355NDT_OK;
      });
  gb.rounds = ls.rounds();
  gb.requests.assign((size_t)K, 0);
  for (int k = 0; k < K; k++) gb.requests[(size_t)k] = ls.requests(k);
  if (!ok) {
    if (round_rc) return round_rc;
    h->err = "gicp_batch_align: a worker thread could not be started";
    return MI355NDT_ERR_HIP;
  }
  for (int k = 0; k < K; k++)
    if (rcs[(size_t)k]) { h->err = where[(size_t)k] + ": the align failed"; return rcs[(size_t)k]; }
  for (int k = 0; k < K; k++) {
    memcpy(gb.slot[(size_t)k].final_cm, fin[(size_t)k].data(), 16 * sizeof(float));
    gb.slot[(size_t)k].have_final = true;
    results[k] = res[(size_t)k];
  }
  return MI355NDT_OK;
}

int mi355ndt_gicp_batch_get_aligned(mi355ndt_handle* h, int slot, void* out_pts, size_t out_stride_bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!out_pts || out_stride_bytes < 12) return MI355NDT_ERR_BAD_ARG;
  GicpBatchSlot* sl;
  int rc = gicp_batch_slot(h, "gicp_batch_get_aligned", slot, &sl);
  if (rc) return rc;
  const std::string where = "gicp_batch_get_aligned: slot " + std::to_string(slot);
  if (!sl->have_final) { h->err = where + ": no batch align has run"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  GicpView S;
  rc = gicp_view_side(h, sl->side, where.c_str(), " is unset", &S);
  if (rc) return rc;
  return gicp_move_out(h, S, sl->final_cm, out_pts, out_stride_bytes);
}

int mi355ndt_gicp_batch_stats(mi355ndt_handle* h, int* rounds, int* requests) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  auto& gb = h->gicp_batch;
  if (gb.slot.empty()) { h->err = "gicp_batch_stats: no slots are reserved (mi355ndt_gicp_batch_reserve first)"; return MI355NDT_ERR_STATE; }
  if (rounds) *rounds = gb.rounds;
  if (requests)
    for (size_t k = 0; k < gb.slot.size(); k++) requests[k] = gb.requests[k];
  return MI355NDT_OK;
}
