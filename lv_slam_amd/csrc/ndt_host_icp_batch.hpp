// ndt_host_icp_batch.hpp -- mi355ndt_icp_batch_*: every ICP candidate of one loop check against the surface's target, aligned in one batch
// (the loop detector's per-candidate loop, loop_detector.hpp:148-205, :211-281).  ICP has no inner optimiser: one iteration is one device
// round trip, so the lockstep is a plain loop on the calling thread -- icp_outer (icp_outer.hpp), the loop the single-pair surface runs
// with K = 1 -- with no worker threads and no rendezvous.  A round: the table of the slots that have not ended (pinned twin -> device, in
// the stream), k_icp_step_batch, k_icp_final_batch, one wait (ndt_icp.hpp, 3); then each slot's SVD and criteria on the host.  The kernels'
// bodies and the host loop are the single-pair surface's, so every slot's result is that surface's, byte for byte.  The single-pair surface
// (its clouds, working cloud, last run), the GICP and NDT surfaces, the grids and the keyframes' rows are left as they were.
#pragma once

typedef mi355ndt_handle::IcpBatch::Slot IcpBatchSlot;

static int icp_batch_slot(mi355ndt_handle* h, const char* where, int slot, IcpBatchSlot** out) {
  auto& ib = h->icp_batch;
  if (ib.slot.empty()) { h->err = std::string(where) + ": no slots are reserved (mi355ndt_icp_batch_reserve first)"; return MI355NDT_ERR_STATE; }
  if (slot < 0 || slot >= (int)ib.slot.size()) {
    h->err = std::string(where) + ": slot " + std::to_string(slot) + " outside 0.." + std::to_string(ib.slot.size() - 1);
    return MI355NDT_ERR_BAD_ARG;
  }
  *out = &ib.slot[(size_t)slot];
  return MI355NDT_OK;
}

int mi355ndt_icp_batch_reserve(mi355ndt_handle* h, int n_slots) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (n_slots < 1 || n_slots > MI355NDT_ICP_BATCH_MAX) {
    h->err = "icp_batch_reserve: n_slots outside 1.." + std::to_string(MI355NDT_ICP_BATCH_MAX);
    return MI355NDT_ERR_BAD_ARG;
  }
  auto& ib = h->icp_batch;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));     // nothing enqueued may still read what the earlier slots own
  ib.slot.clear();
  ib.rounds = 0; ib.requests.assign((size_t)n_slots, 0);
  HIPCHK(h, ib.m.reserve(MI355NDT_ICP_BATCH_MAX));
  HIPCHK(h, ib.d_tab.reserve(MI355NDT_ICP_BATCH_MAX));
  HIPCHK(h, ib.h_tab.reserve(MI355NDT_ICP_BATCH_MAX));
  if (!ib.h_rec) {
    HIPCHK(h, ib.h_rec.reserve((size_t)MI355NDT_ICP_BATCH_MAX * ICP_REC, hipHostMallocMapped));
    ib.d_rec = ib.h_rec.dev();
    if (!ib.d_rec) { ib.h_rec = PinBuf<double>(); h->err = "icp_batch_reserve: no device view of the mapped result records"; return MI355NDT_ERR_HIP; }
  }
  ib.slot.resize((size_t)n_slots);
  return MI355NDT_OK;
}

int mi355ndt_icp_batch_set_source(mi355ndt_handle* h, int slot, const void* pts, size_t n, size_t stride_bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  IcpBatchSlot* sl;
  int rc = icp_batch_slot(h, "icp_batch_set_source", slot, &sl);
  if (rc) return rc;
  sl->work.have_final = false;
  return gicp_side_set_host(h, sl->side, pts, n, stride_bytes);
}

int mi355ndt_icp_batch_set_source_keyframe(mi355ndt_handle* h, int slot, int id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  IcpBatchSlot* sl;
  int rc = icp_batch_slot(h, "icp_batch_set_source_keyframe", slot, &sl);
  if (rc) return rc;
  if (!kf_find(h, id, "icp_batch_set_source_keyframe")) return MI355NDT_ERR_BAD_ARG;
  sl->side.kf_id = id; sl->side.set = true;
  sl->work.have_final = false;
  return MI355NDT_OK;
}

// the batch's evaluator of icp_outer: one round for the slots that have not ended -- one table copy, two launches, one wait.  After a failed
// round icp_outer launches nothing more and returns the error.
struct IcpEvalBatch {
  mi355ndt_handle* h; const GicpView& D; const std::vector<GicpView>& S;
  int step(const int* slots, int n, const IcpRun* runs, IcpSums* sums) {
    auto& ib = h->icp_batch;
    hipStream_t s = h->stream;
    IcpSlot* tab = ib.h_tab;
    int chunks = 0;
    for (int j = 0; j < n; j++) {
      const int k = slots[j];
      const GicpView& v = S[(size_t)k];
      auto& w = ib.slot[(size_t)k].work;
      IcpSlot& e = tab[j];
      e.in = runs[k].first ? v.rows : (const float*)w.W; e.W = w.W;
      e.idx = w.idx; e.d2 = w.d2; e.m = ib.m + k; e.part = w.part;
      e.rec = ib.d_rec + (size_t)k * ICP_REC;
      e.pitch = (unsigned)v.pitch; e.n = (int)v.n;
      e.n_chunks = (int)((v.n + GC_CHUNK - 1) / GC_CHUNK);
      e.chunk0 = chunks; chunks += e.n_chunks;
      e.step = icp_make_step(h->icp.prm, nullptr, runs[k].T);
    }
    HIPCHK(h, hipMemcpyAsync(ib.d_tab, tab, (size_t)n * sizeof(IcpSlot), hipMemcpyHostToDevice, s));
    k_icp_step_batch<<<(unsigned)chunks, GC_CHUNK, 0, s>>>(ib.d_tab, n, kfi_view(*D.index, D.rows, D.pitch, D.n));
    k_icp_final_batch<<<(unsigned)n, 256, 0, s>>>(ib.d_tab);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    for (int j = 0; j < n; j++) {
      const int k = slots[j];
      for (int i = 0; i < ICP_SUMS; i++) sums[k].v[i] = ib.h_rec[(size_t)k * ICP_REC + i];
      sums[k].m = (int)ib.h_rec[(size_t)k * ICP_REC + ICP_SUMS];
    }
    return MI355NDT_OK;
  }
};

int mi355ndt_icp_batch_align(mi355ndt_handle* h, const float* guesses_colmajor, mi355ndt_icp_result* results) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!guesses_colmajor || !results) return MI355NDT_ERR_BAD_ARG;
  auto& ib = h->icp_batch;
  const int K = (int)ib.slot.size();
  if (!K) { h->err = "icp_batch_align: no slots are reserved (mi355ndt_icp_batch_reserve first)"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  GicpView D;
  std::vector<GicpView> S((size_t)K);
  int rc = MI355NDT_OK;
  for (int k = 0; k < K && !rc; k++) {              // (the views first: a refused batch has built nothing)
    const std::string where = "icp_batch_align: slot " + std::to_string(k);
    rc = gicp_view_side(h, ib.slot[(size_t)k].side, where.c_str(), " is unset", &S[(size_t)k]);
  }
  if (!rc) rc = icp_target(h, "icp_batch_align", &D);
  for (int k = 0; k < K && !rc; k++) {
    const std::string where = "icp_batch_align: slot " + std::to_string(k);
    rc = icp_source(h, ib.slot[(size_t)k].side, ib.slot[(size_t)k].work, where.c_str(), " is unset", &S[(size_t)k]);
  }
  if (rc) return rc;
  HIPCHK(h, hipMemsetAsync(ib.m, 0, MI355NDT_ICP_BATCH_MAX * sizeof(int), h->stream));   // (a failed round may have left a count behind)
  IcpEvalBatch ev{h, D, S};
  std::vector<IcpRun> runs;
  ib.requests.assign((size_t)K, 0);
  rc = icp_outer(ev, h->icp.prm, K, guesses_colmajor, runs, &ib.rounds, ib.requests.data());
  if (rc) return rc;
  for (int k = 0; k < K; k++) {
    ib.slot[(size_t)k].work.run = runs[(size_t)k];
    ib.slot[(size_t)k].work.have_final = true;
    icp_result(runs[(size_t)k], &results[k]);
  }
  return MI355NDT_OK;
}

int mi355ndt_icp_batch_get_aligned(mi355ndt_handle* h, int slot, void* out_pts, size_t out_stride_bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!out_pts || out_stride_bytes < 12) return MI355NDT_ERR_BAD_ARG;
  IcpBatchSlot* sl;
  int rc = icp_batch_slot(h, "icp_batch_get_aligned", slot, &sl);
  if (rc) return rc;
  if (!sl->work.have_final) { h->err = "icp_batch_get_aligned: slot " + std::to_string(slot) + ": no batch align has run"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return icp_work_out(h, sl->work, out_pts, out_stride_bytes);
}

int mi355ndt_icp_batch_stats(mi355ndt_handle* h, int* rounds, int* requests) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  auto& ib = h->icp_batch;
  if (ib.slot.empty()) { h->err = "icp_batch_stats: no slots are reserved (mi355ndt_icp_batch_reserve first)"; return MI355NDT_ERR_STATE; }
  if (rounds) *rounds = ib.rounds;
  if (requests)
    for (size_t k = 0; k < ib.slot.size(); k++) requests[k] = ib.requests[k];
  return MI355NDT_OK;
}
