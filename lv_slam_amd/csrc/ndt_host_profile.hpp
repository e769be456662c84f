// ndt_host_profile.hpp -- profiling: the pooled timing events around sweeps, updates and builds (ev_*), mi355ndt_profile_*.
#pragma once

// ---- profiling helpers ------------------------------------------------------------------------
// timing events come from a pool that mi355ndt_profile_enable fills up front: creating events inside a timed region can
// stall for milliseconds when the runtime has to grow its signal pool
static hipError_t ev_take(mi355ndt_handle* h, hipEvent_t* e) {
  if (!h->ev_pool.empty()) { *e = h->ev_pool.back(); h->ev_pool.pop_back(); return hipSuccess; }
  return hipEventCreate(e);
}
// Back-to-back kernels share an event: the end of one span is the begin of the next (half the event records in the round loop).
static hipError_t ev_begin(mi355ndt_handle* h, std::vector<mi355ndt_handle::EvSpan>& v) {
  if (h->ev_last_fresh && h->ev_last) {
    v.push_back({h->ev_last, nullptr, true});
    h->ev_last_fresh = false;
    return hipSuccess;
  }
  hipEvent_t a;
  hipError_t e = ev_take(h, &a); if (e != hipSuccess) return e;
  v.push_back({a, nullptr, false});
  return hipEventRecord(a, h->stream);
}
static hipError_t ev_end(mi355ndt_handle* h, std::vector<mi355ndt_handle::EvSpan>& v) {
  hipEvent_t b;
  hipError_t e = ev_take(h, &b); if (e != hipSuccess) return e;
  v.back().second = b;
  h->ev_last = b;
  h->ev_last_fresh = true;
  return hipEventRecord(b, h->stream);
}
static void ev_collect(mi355ndt_handle* h, std::vector<mi355ndt_handle::EvSpan>& v, double& ms, long long& n) {
  for (auto& e : v) {
    float t = 0;
    if (e.second && hipEventElapsedTime(&t, e.first, e.second) == hipSuccess) { ms += t; n++; }
    if (!e.first_shared) h->ev_pool.push_back(e.first);
    if (e.second) h->ev_pool.push_back(e.second);
  }
  v.clear();
  h->ev_last_fresh = false;
}
int mi355ndt_profile_enable(mi355ndt_handle* h, int on) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  h->prof = on != 0;
  if (h->ss) for (int c = 0; c < h->ss->nctx; c++) if (h->ss->ctx[c].e) { h->ss->ctx[c].e->ev_pool_target = 128; (void)mi355ndt_profile_enable(h->ss->ctx[c].e.get(), on); }
  if (h->prof) {
    HIPCHK(h, hipSetDevice(h->device));
    while (h->ev_pool.size() < h->ev_pool_target) { // ~40 profiled steps of a 10-round batch align before the pool has to grow
      hipEvent_t e;
      HIPCHK(h, hipEventCreate(&e));
      h->ev_pool.push_back(e);
    }
  }
  return MI355NDT_OK;
}
int mi355ndt_profile_reset(mi355ndt_handle* h) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  double d; long long n;
  ev_collect(h, h->ev_sweep, d, n); ev_collect(h, h->ev_update, d, n); ev_collect(h, h->ev_build, d, n);
  if (h->ss) for (int c = 0; c < h->ss->nctx; c++) if (mi355ndt_handle* e = h->ss->ctx[c].e.get()) {
    ev_collect(e, e->ev_sweep, d, n); ev_collect(e, e->ev_update, d, n); ev_collect(e, e->ev_build, d, n);
    e->P = mi355ndt_profile{};
  }
  h->P = mi355ndt_profile{};
  (void)hipMemsetAsync(h->d_hits, 0, 2 * sizeof(unsigned long long), h->stream);
  (void)hipStreamSynchronize(h->stream);
  return MI355NDT_OK;
}
int mi355ndt_profile_get(mi355ndt_handle* h, mi355ndt_profile* out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!out) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ev_collect(h, h->ev_sweep, h->P.sweep_ms, h->P.sweep_launches);
  ev_collect(h, h->ev_update, h->P.update_ms, h->P.update_launches);
  ev_collect(h, h->ev_build, h->P.build_ms, h->P.build_launches);
  if (h->ss) for (int c = 0; c < h->ss->nctx; c++) if (mi355ndt_handle* e = h->ss->ctx[c].e.get()) {   // the contexts' builds (and synchronous re-runs) are this handle's work
    ev_collect(e, e->ev_sweep, h->P.sweep_ms, h->P.sweep_launches);
    ev_collect(e, e->ev_update, h->P.update_ms, h->P.update_launches);
    ev_collect(e, e->ev_build, h->P.build_ms, h->P.build_launches);
    h->P.build_alg_bytes += e->P.build_alg_bytes; e->P.build_alg_bytes = 0;
    { std::lock_guard<std::mutex> lk(e->up_mtx);   // (mi355ndt_stream_submit_host stages into the contexts' engines)
      h->P.cloud_uploads += e->P.cloud_uploads; e->P.cloud_uploads = 0; h->P.cloud_upload_bytes += e->P.cloud_upload_bytes; e->P.cloud_upload_bytes = 0;
      h->P.cloud_transfers += e->P.cloud_transfers; e->P.cloud_transfers = 0; }
  }
  unsigned long long hh[2] = {0, 0};              // (point, voxel) evaluations and score-only sweeps since the last reset, summed on the device
  HIPCHK(h, hipMemcpy(hh, h->d_hits, sizeof hh, hipMemcpyDeviceToHost));
  *out = h->P;
  if (h->ss) { out->stream_reserved_slots = h->ss->last_reserve; out->stream_launch_slots = h->ss->last_slots; }
  out->sweep_hits += (long long)hh[0];
  out->sweep_alg_bytes += 64.0 * (double)hh[0];
  out->score_only_sweeps = (long long)hh[1];
  out->async_waves_per_simd = h->last_async_wpe; out->async_launch_slots = h->last_async_grid;
  return MI355NDT_OK;
}
