// ndt_host_align.hpp -- the aligns: mi355ndt_batch_align over its three paths (one persistent launch, latency-mode pump, lockstep rounds), their
// common end, pose records, and the single-registration surface on pair slot 0.
#pragma once
// MI355NDT_OPT_ARITH = 1: results of registrations the tolerance arithmetic is not meant for carry a warning (include/mi355_ndt.h).  A property of the
// pair alone (its hits at the final pose, its iteration count), applied to the host copy of the results by every path that hands results out.
static void tolerance_warnings(const mi355ndt_handle* h, mi355ndt_result* out, int n) {
  if (!fast_served(h)) return;
  for (int b = 0; b < n; b++)
    if (out[b].status == MI355NDT_OK && (out[b].hits_last < MI355NDT_TOLERANCE_MIN_HITS || out[b].iterations >= h->prm.max_iterations + 2))
      out[b].status = MI355NDT_WARN_TOLERANCE_ARITH;
}
static int ensure_seq_flags(mi355ndt_handle* h) {
  if (!h->d_seq_flags) {
    HIPCHK(h, h->h_seq_flags.reserve(16, hipHostMallocMapped | hipHostMallocCoherent));   // fine-grained: device writes are visible to the polling host
    if (!(h->d_seq_flags = h->h_seq_flags.dev())) { h->err = "hipHostGetDevicePointer failed"; return MI355NDT_ERR_HIP; }
  }
  return MI355NDT_OK;
}

// Latency mode's Newton loop: (update, sweep) rounds enqueued at most `depth` ahead of the sweep the device last reported from;
// every fine sweep writes "pairs still active" and its sequence number into mapped host memory, so the loop needs neither the
// per-burst counter copy nor an event wait.  Ends when a sweep reports that no pair is active.
static int align_pump(mi355ndt_handle* h, SweepConst sc, int B) {
  int rc = ensure_seq_flags(h);
  if (rc) return rc;
  hipStream_t s = h->stream;
  h->h_seq_flags[0] = 0; h->h_seq_flags[1] = -1;
  sc.host_flags = h->d_seq_flags;
  sc.seq_no = 1;
  sc.rebase_block = 1;                           // every fine sweep also prepares the next update's re-basing (its extra workgroup)
  rc = launch_sweep(h, sc);                      // the sweep at the guess
  if (rc) return rc;
  const int depth = 2;
  const long long max_rounds = h->prm.max_iterations + 4;
  long long enq = 0;                             // (update, sweep) rounds enqueued; sweep of round r carries seq_no r + 1
  auto t_progress = std::chrono::steady_clock::now();
  long long seen_last = -1;
  for (;;) {
    const long long seen = h->h_seq_flags[0];    // sequence number of the last sweep that has started
    const int active = h->h_seq_flags[1];
    if (seen >= 1 && active == 0) break;         // that sweep found nothing to do: every pair is finalised
    if (seen != seen_last) { seen_last = seen; t_progress = std::chrono::steady_clock::now(); }
    if (enq >= max_rounds || enq + 1 - seen >= depth) {
      if (std::chrono::steady_clock::now() - t_progress > std::chrono::seconds(20)) { h->err = "align: the device stopped making progress"; return MI355NDT_ERR_STATE; }
      cpu_relax();                               // (busy-wait: a round is ~20 us, a yield costs more than it gives; pause frees the sibling hyperthread)
      continue;
    }
    k_update<<<B, UPD_THREADS, 0, s>>>(h->d_state, h->d_partials, h->rows_per_pair, h->pts_per_chunk, 1, h->d_results, h->d_active,
                                       h->d_active_list, h->d_ctl + h->ctl_idx, h->prof ? h->d_hits : nullptr, h->prm.step_size, h->prm.trans_epsilon,
                                       h->prm.max_iterations, 0, 0, nullptr, nullptr, 0);
    sc.seq_no = (int)(enq + 2);
    rc = launch_sweep(h, sc);
    if (rc) return rc;
    enq++;
  }
  return MI355NDT_OK;
}

// profile accounting of finished aligns: every sweep a pair took part in streamed its points + K table probes
static void account_sweeps(mi355ndt_handle* h, const mi355ndt_result* out, const int* src_cnt, int n, int K) {
  if (!h->prof) return;
  for (int b = 0; b < n; b++) {
    h->P.sweep_alg_bytes += sweep_alg_bytes((double)out[b].sweeps * src_cnt[b], K);
    h->P.sweep_points += (long long)out[b].sweeps * src_cnt[b];
  }
}
// The end of every align path: the results down, the stream drained, the launches' errors surfaced, the sweeps' bytes accounted, the batch marked
// as aligned.  `account` = false: the path has accounted already (the rounds do, burst by burst).  `launch`: the one-launch align's control block
// (its copy is already enqueued) -- a launch that gave up or left pairs unfinished ends here with MI355NDT_ERR_UNSUPPORTED and nothing marked.
static int finish_align(mi355ndt_handle* h, const SweepConst& sc, int B, mi355ndt_result* out, bool account, const AsyncCtl* launch = nullptr) {
  HIPCHK(h, hipMemcpyAsync(out, h->d_results, (size_t)B * sizeof(mi355ndt_result), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  if (launch && (launch->abort_ || launch->fin != (unsigned)B)) {
    // a wave gave up (its ticket never came within the poll budget: a device shared with something that starves the launch, or the
    // test hook): nothing is lost -- the round-based path produces the same bits from the same guesses
    h->P.async_fallbacks++;
    return MI355NDT_ERR_UNSUPPORTED;
  }
  if (account) account_sweeps(h, out, h->h_src_cnt.data(), B, sc.K);
  h->aligned_once = true;
  return MI355NDT_OK;
}

static int align_async(mi355ndt_handle* h, const SweepConst& sc, int B, mi355ndt_result* out, bool lean) {
  const int ring_cap = async_ring_cap(h, B);
  if (ring_cap == 0) return MI355NDT_ERR_UNSUPPORTED;
  // (a ring that cannot be allocated is no error of the align: the round-based path needs none)
  if (h->d_ring.reserve((size_t)8 * ring_cap) != hipSuccess) { (void)hipGetLastError(); return MI355NDT_ERR_UNSUPPORTED; }
  HIPCHK(h, h->d_arrived.reserve((size_t)B * ASYNC_ARR_STRIDE));
  HIPCHK(h, h->d_actl.reserve(1));
  HIPCHK(h, h->d_atab.reserve(1));
  HIPCHK(h, h->h_pin_actl.reserve(1));
  // everything the launch polls is reset on the stream before it (never inside the kernel, never by a previous launch), together with
  // the pairs' initial states
  AsyncLaunch L;
  memset(&L.tab, 0, sizeof L.tab);
  fill_async_ctx(h, L.tab.c[0]);
  L.new_ci = 0; L.n_new = B;
  L.st_new = h->d_state; L.guess_new = h->d_guess; L.src_cnt_new = h->d_src_cnt; L.gd_new = h->d_grid; L.arrived_new = h->d_arrived;
  L.active_list = h->d_active_list; L.sweep_ctl = h->d_ctl;
  L.tab_dev = h->d_atab; L.ring = h->d_ring; L.ring_cap = ring_cap; L.ctl = h->d_actl; L.prev = nullptr;
  L.items_per_pair = h->items_per_pair; L.stop_thresh = 0; L.debug_abort_pos = h->debug_abort_pos; L.debug_ring_mask = h->debug_ring_mask;
  L.lean = lean;
  int rc = launch_async(h, sc, L);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(h->h_pin_actl, h->d_actl, 8 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));   // pub, fin, abort_, n_live, susp
  return finish_align(h, sc, B, out, true, h->h_pin_actl.p);
}

static int batch_align_impl(mi355ndt_handle* h, const float* guesses, mi355ndt_result* out) {
  if (!guesses || !out) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs <= 0 || !h->d_tgt || !h->d_src) return MI355NDT_ERR_STATE;
  const bool mt_live = mt_is_live(h->prm);                       // impl2:888: More-Thuente loop + computeHessian are live
  if (const char* why = model_refuses(h->prm, h->pose_model, h->ndt_class, h->ground_class)) { h->err = why; return MI355NDT_ERR_UNSUPPORTED; }   // (nothing touched)
  int rc = ensure_grids(h, GRIDS_CONFIG);
  if (rc) return rc;
  rc = prep_align_ws(h);
  if (rc) return rc;
  const int B = h->n_pairs;
  hipStream_t s = h->stream;
  SweepConst sc;
  make_sweep_const(h, sc);
  gauss_constants3(h->prm.outlier_ratio, h->prm.resolution, h->gauss_last);     // computeTransformation sets the members (impl2:93-100)
  // the engine's stream is idle here (every entry point returns synchronised), so the pinned staging copy is free to overwrite
  h->ev_last_fresh = false;
  memcpy(h->h_pin_guess, guesses, (size_t)B * 16 * sizeof(float));
  HIPCHK(h, hipMemcpyAsync(h->d_guess, h->h_pin_guess, (size_t)B * 16 * sizeof(float), hipMemcpyHostToDevice, s));
  h->ctl_idx = 0;
  // One launch for the whole align (ndt_async.hpp) when the batch offers more work items than the GPU has resident waves.  A smaller batch
  // -- a single registration above all -- keeps the round-based kernels, whose flat dealing spreads a pair's items over every XCD: a ticket
  // is served by ONE ring (an eighth of the waves), which costs a lone 65,536-point pair 0.39 ms against 0.31 ms per align.
  // (two or three waves per SIMD: decided here, once per launch, from the batch's largest target -- async_lean, ndt_host_sweep.hpp)
  const int tgt_max = *std::max_element(h->h_tgt_cnt.begin(), h->h_tgt_cnt.begin() + B);
  const bool lean = async_lean(h, sc, sweep_ord(h, sc), tgt_max > 0 ? (size_t)tgt_max : h->tgt_pitch);   // (counts the host never saw: the rows' pitch bounds them)
  // (which path a batch takes does not follow that choice: "more work items than resident waves" is asked of the geometry every configuration has)
  const bool big_batch = (long long)B * h->items_per_pair > (long long)launch_slots(h, sc, sweep_ord(h, sc) == 2) * WAVES;
  if (async_served(h) && (big_batch || h->async_force) && !h->fine_it) {
    rc = align_async(h, sc, B, out, lean);                                // (prepares the pair states itself: k_async_prepare)
    if (rc != MI355NDT_ERR_UNSUPPORTED) return rc;                  // done, or failed.  (Not resident, no ring, or the launch gave up: the lockstep rounds below)
  }
  HIPCHK(h, hipMemsetAsync(h->d_ctl, 0, 2 * sizeof(SweepCtl), s));
  k_init_state<<<(B + 63) / 64, 64, 0, s>>>(h->d_state, h->d_guess, h->d_src_cnt, h->d_grid, B, h->d_active_list, h->d_ctl, euler_rows_of(h), pcl_rows_of(h));
  if (h->fine_it) {                                // latency mode: the pump (no bursts, no counter copies, no event waits)
    rc = align_pump(h, sc, B);
    return rc ? rc : finish_align(h, sc, B, out, true);
  }
  rc = launch_sweep(h, sc);
  if (rc) return rc;
  const int max_rounds = h->prm.max_iterations + 4;   // loop body runs for it = 0 .. max_iterations+1
  double pts_total = 0;
  for (int b = 0; b < B; b++) pts_total += h->h_src_cnt[b];
  const double alg_static = sweep_alg_bytes(pts_total, sc.K);   // every active pair streams its points + K table probes
  if (h->prof) {
    h->P.sweep_alg_bytes += alg_static;                          // the initial sweep covers all pairs
    h->P.sweep_points += (long long)pts_total;
  }
  // update+sweep rounds are enqueued in bursts of two; the host always keeps ONE burst queued ahead of the one whose
  // "pairs still active" counters it is waiting for, so the device never idles over a host round trip.  The price is
  // at most one speculative burst after the last pair finished (k_update / k_sweep return at once with nothing active).
  const int burst = 2;
  int round = 0, n_enq = 0;
  int cnt[2] = {0, 0};                                           // rounds in the burst held by ring slot 0 / 1
  auto enqueue_burst = [&]() -> int {
    const int slot = n_enq & 1;
    h->ev_last_fresh = false;                    // the burst bookkeeping below sits between the previous sweep and this update
    int* dact = h->d_active + slot * burst;
    hipError_t e = hipMemsetAsync(dact, 0, burst * sizeof(int), s);
    if (e != hipSuccess) return MI355NDT_ERR_HIP;
    int k = 0;
    for (; k < burst && round < max_rounds; k++, round++) {
      if (h->prof) HIPCHK(h, ev_begin(h, h->ev_update));
      k_update<<<B, UPD_THREADS, 0, s>>>(h->d_state, h->d_partials, h->rows_per_pair, h->pts_per_chunk, h->fine_it ? 1 : 0, h->d_results, dact + k,
                                h->d_active_list, h->d_ctl + h->ctl_idx, h->prof ? h->d_hits : nullptr,
                                h->prm.step_size, h->prm.trans_epsilon, h->prm.max_iterations, 0, mt_live ? 1 : 0, euler_rows_of(h), pcl_rows_of(h), eff_ground(h));
      if (mt_live) {      // pairs whose More-Thuente loop iterated get their Hessian from computeHessian (impl2:999-1000)
        launch_hessian(h, sc);
        k_update<<<B, UPD_THREADS, 0, s>>>(h->d_state, h->d_partials, h->rows_per_pair, h->pts_per_chunk, h->fine_it ? 1 : 0, h->d_results, dact + k,
                                  h->d_active_list, h->d_ctl + h->ctl_idx, nullptr,
                                  h->prm.step_size, h->prm.trans_epsilon, h->prm.max_iterations, 0, 2, nullptr, nullptr, 0);
      }
      if (h->prof) HIPCHK(h, ev_end(h, h->ev_update));
      int r = launch_sweep(h, sc);
      if (r) return r;
    }
    cnt[slot] = k;
    HIPCHK(h, hipMemcpyAsync(h->h_pin_active + slot * burst, dact, burst * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipEventRecord(h->ev_burst[slot], s));
    n_enq++;
    return MI355NDT_OK;
  };
  rc = enqueue_burst();
  if (rc) return rc;
  for (int done = 0; done < n_enq; done++) {
    if (round < max_rounds) { rc = enqueue_burst(); if (rc) return rc; }     // speculative: one burst ahead
    const int slot = done & 1;
    HIPCHK(h, hipEventSynchronize(h->ev_burst[slot]));
    const int* act = h->h_pin_active + slot * burst;
    if (h->prof) {
      // sweep k of this burst streamed the pairs that scheduled a step in update k (equal-size pairs assumed)
      for (int k = 0; k < cnt[slot]; k++) {
        const double frac = (double)act[k] / B;
        h->P.sweep_alg_bytes += alg_static * frac;
        h->P.sweep_points += (long long)(pts_total * frac);
      }
    }
    if (act[cnt[slot] - 1] == 0) break;
  }
  // (the device-side hit counter d_hits keeps accumulating; mi355ndt_profile_get reads it -- every sweep is followed by an
  //  update, which is where the hits are added, so nothing is missing when the loop exits)
  return finish_align(h, sc, B, out, false);
}

int mi355ndt_batch_align(mi355ndt_handle* h, const float* guesses, mi355ndt_result* out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  const int rc = batch_align_impl(h, guesses, out);
  if (rc == MI355NDT_OK) tolerance_warnings(h, out, h->n_pairs);
  if (rc != MI355NDT_OK) {
    // an error exit may leave (update, sweep) rounds queued: drain them, so that no sweep of THIS align can post its progress words
    // into the flags the next align resets (the latency-mode pump restarts its sequence numbers at 1)
    (void)hipStreamSynchronize(h->stream);
    if (h->ev_compute) (void)compute_enqueued(h);                         // see mi355ndt_batch_build_targets
  }
  return rc;
}
int mi355ndt_batch_pose_records(mi355ndt_handle* h, int id_base, int id_stride, void* d_records, size_t capacity) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!d_records || capacity == 0 || capacity > (size_t)MAX_PAIRS || (size_t)h->n_pairs > capacity) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs <= 0 || !h->d_results || !h->aligned_once) return MI355NDT_ERR_STATE;   // no align of this batch yet: nothing to pack
  HIPCHK(h, hipSetDevice(h->device));
  static_assert(sizeof(PoseRecord) == 96, "pose record is 96 bytes");
  k_pose_records<<<(unsigned)((capacity + 255) / 256), 256, 0, h->stream>>>(h->d_results, h->n_pairs, id_base, id_stride, (PoseRecord*)d_records, (int)capacity);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MI355NDT_OK;
}

// ---- single-registration surface (pair slot 0) ---------------------------------------------------
static int ensure_single(mi355ndt_handle* h, bool tgt, size_t n) {
  const size_t want = std::max(((n + 63) & ~(size_t)63), (size_t)64);
  const bool single = h->n_pairs == 1 && h->d_tgt_own && h->d_src_own && h->d_tgt == h->d_tgt_own && h->d_src == h->d_src_own;
  if (!single) {
    // leaving batch / bound mode: start a fresh one-pair engine
    return mi355ndt_batch_reserve(h, 1, tgt ? want : 64, tgt ? 64 : want);
  }
  // target and source buffers are independent: grow only the side being replaced
  const size_t have = tgt ? h->own_tgt_pitch : h->own_src_pitch;
  if (n <= have) return MI355NDT_OK;
  int rc = alloc_side(h, tgt, 1, want);
  if (rc) return rc;
  if (tgt) h->tgt_pitch = want; else h->src_pitch = want;
  h->d_tgt = h->d_tgt_own; h->d_src = h->d_src_own;
  return MI355NDT_OK;
}

// setInputTarget / setInputSource of the one-pair engine: make room on that side, upload
static int set_single(mi355ndt_handle* h, bool tgt, const void* pts, size_t n, size_t stride) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if ((!pts && n) || (n && stride < 12) || n >= (1u << 31)) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const int rc = ensure_single(h, tgt, n);
  return rc ? rc : batch_set_side(h, tgt, 0, pts, n, stride);
}
int mi355ndt_set_target(mi355ndt_handle* h, const void* pts, size_t n, size_t stride) {
  const int rc = set_single(h, true, pts, n, stride);
  return rc ? rc : mi355ndt_batch_build_targets(h);      // init(): filter(true) (ndt_omp.h:270-277)
}
int mi355ndt_set_source(mi355ndt_handle* h, const void* pts, size_t n, size_t stride) { return set_single(h, false, pts, n, stride); }

int mi355ndt_align(mi355ndt_handle* h, const float guess[16], mi355ndt_result* out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!guess || !out) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs < 1 || !h->have_target || !h->have_source) return MI355NDT_ERR_STATE;
  if (h->n_pairs != 1) return MI355NDT_ERR_STATE;                   // a batch is bound: use mi355ndt_batch_align
  // pcl::Registration::initCompute() refuses empty clouds; align() then returns without touching converged_
  if (h->h_tgt_cnt[0] <= 0 || h->h_src_cnt[0] <= 0) return MI355NDT_ERR_STATE;
  int rc = mi355ndt_batch_align(h, guess, out);
  if (rc == MI355NDT_OK) memcpy(h->last_final, out->final_colmajor, sizeof h->last_final);
  return rc;
}

// The nodelet's keyframe switch (scan_matching_odom_nodelet.cpp:240-243: `key = filtered; reg_s2k.setInputTarget(key);`) makes the cloud that was
// just aligned as SOURCE the next target: it is on the device already -- device-to-device into the target rows, then init() as setInputTarget does.
int mi355ndt_promote_source_to_target(mi355ndt_handle* h) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (h->n_pairs != 1 || !h->have_source || h->d_src != h->d_src_own || !h->d_src_own) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t m = (size_t)h->h_src_cnt[0];
  int rc = ensure_single(h, true, m);
  if (rc) return rc;
  rc = rows_into_slot(h, true, 0, h->d_src_own, h->src_pitch, m);
  if (rc) return rc;
  h->P.cloud_promotions++;
  return mi355ndt_batch_build_targets(h);
}
