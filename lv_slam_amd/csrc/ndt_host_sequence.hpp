// ndt_host_sequence.hpp -- latency mode's switch and the sequence run: a whole scan-to-keyframe sequence pumped without a host decision per frame.
#pragma once

// ---- latency mode ---------------------------------------------------------------------------------------------------------
int mi355ndt_set_latency_mode(mi355ndt_handle* h, int on) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  h->latency_mode = on != 0;
  return MI355NDT_OK;
}

// what both sequence runs ask of the handle and of their common arguments
static int sequence_args(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride, const double* stamps,
                         mi355ndt_seq_frame* out_frames, size_t count_limit, size_t* maxn) {
  if (n_frames < 1 || n_frames > MAX_PAIRS || !clouds || !counts || !stamps || !out_frames || stride < 12) return MI355NDT_ERR_BAD_ARG;
  if (mt_is_live(h->prm) || (h->prm.neighbor_mode != MI355NDT_DIRECT1 && h->prm.neighbor_mode != MI355NDT_DIRECT7)) {
    h->err = "sequence mode serves DIRECT1 / DIRECT7 with step_size > transformation_epsilon / 2 (every configuration lv_slam ships)";
    return MI355NDT_ERR_UNSUPPORTED;
  }
  *maxn = 0;
  for (int k = 0; k < n_frames; k++) { if (counts[k] == 0 || counts[k] >= count_limit || !clouds[k]) return MI355NDT_ERR_BAD_ARG; *maxn = std::max(*maxn, counts[k]); }
  return MI355NDT_OK;
}

// The run itself, from the point where the n_frames frames sit in target slots 0 .. n_frames - 1 of the engine's own batch (recorded with their
// counts); upload_ms: what getting them there took.
static int sequence_tracked(mi355ndt_handle* h, int n_frames, const double* stamps, const mi355ndt_seq_params* policy,
                            mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results, mi355ndt_seq_stats* stats, double upload_ms) {
  int rc;
  const std::vector<int> counts(h->h_tgt_cnt.begin(), h->h_tgt_cnt.begin() + n_frames);
  h->d_src = h->d_tgt_own; h->src_pitch = h->tgt_pitch;
  cloud_changed(h, false, 0, n_frames, counts.data());
  struct Unalias { mi355ndt_handle* h; ~Unalias() { h->d_src = h->d_src_own; h->src_pitch = h->own_src_pitch; clouds_reset(h, false, true);
                                                     h->d_grid_of_use = nullptr; h->aligned_once = false;
                                                     if (h->ev_compute) (void)compute_enqueued(h); } } unalias{h};   // (error exits too: later uploads wait for what was enqueued)
  const bool keep_prof = h->prof;
  struct ProfBack { mi355ndt_handle* h; bool v; ~ProfBack() { h->prof = v; } } profback{h, keep_prof};   // (every exit restores it)
  h->prof = false;
  HipEvent ev[3];
  for (auto& e : ev) HIPCHK(h, e.create(hipEventDefault));
  hipStream_t s = h->stream;
  HIPCHK(h, hipEventRecord(ev[0], s));
  rc = mi355ndt_batch_build_targets(h);
  if (rc) { h->prof = keep_prof; return rc; }
  HIPCHK(h, hipEventRecord(ev[1], s));
  const bool lat = h->latency_mode;
  h->latency_mode = true; h->seq_running = true;
  rc = prep_align_ws(h);
  h->latency_mode = lat; h->seq_running = false;
  if (rc == MI355NDT_OK && !h->fine_it) { h->err = "sequence run: the fine-grained sweep does not serve this configuration"; rc = MI355NDT_ERR_UNSUPPORTED; }
  if (rc) { h->prof = keep_prof; return rc; }
  // one pair is in flight at a time: the fine grid is sized for one pair
  HIPCHK(h, h->d_grid_of.reserve(n_frames)); HIPCHK(h, h->d_seq_out.reserve(n_frames)); HIPCHK(h, h->d_stamps.reserve(n_frames));
  HIPCHK(h, h->d_seq.reserve(1));
  rc = ensure_seq_flags(h);
  if (rc) { h->prof = keep_prof; return rc; }
  h->h_seq_flags[0] = 0; h->h_seq_flags[1] = 0;
  SeqState q0;
  memset(&q0, 0, sizeof q0);
  q0.n_frames = n_frames;
  q0.d_trans = policy ? policy->keyframe_delta_trans : 5.0;                       // scan_matching_odom_nodelet.cpp:67-76
  q0.d_angle = policy ? policy->keyframe_delta_angle : 0.17;
  q0.d_time = policy ? policy->keyframe_delta_time : 1.0;
  HIPCHK(h, hipMemcpyAsync(h->d_seq, &q0, sizeof q0, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->d_stamps, stamps, (size_t)n_frames * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemsetAsync(h->d_grid_of, 0, (size_t)n_frames * sizeof(int), s));
  HIPCHK(h, hipMemsetAsync(h->d_results, 0, (size_t)n_frames * sizeof(mi355ndt_result), s));
  HIPCHK(h, hipMemsetAsync(h->d_ctl, 0, 2 * sizeof(SweepCtl), s));
  HIPCHK(h, hipStreamSynchronize(s));            // q0 / stamps are pageable: they must be out of the caller's memory before the pump starts
  h->ctl_idx = 0;
  h->d_grid_of_use = h->d_grid_of;
  SweepConst sc;
  make_sweep_const(h, sc);
  sc.rebase_block = 1;                           // every fine sweep also prepares the next update's re-basing (its extra workgroup)
  gauss_constants3(h->prm.outlier_ratio, h->prm.resolution, h->gauss_last);
  k_seq_begin<<<1, 64, 0, s>>>(h->d_seq, h->d_state, h->d_grid, h->d_src_cnt, h->d_stamps, h->d_seq_out, h->d_active_list, h->d_ctl, h->d_grid_of, h->d_seq_flags);
  bool stuck = false;
  rc = launch_sweep(h, sc, 1);
  // The pump: (update, sweep), (update, sweep), ... enqueued blindly, at most `depth` rounds ahead of what the device has executed;
  // whether a launch continues a frame's Newton loop, closes the frame and opens the next, or has nothing left to do is decided
  // on the device.  The host never waits for a result -- it only reads two words the device writes into mapped memory.
  const int depth = 12;
  long long enq = 0;
  const long long max_launches = (long long)n_frames * (h->prm.max_iterations + 6) + 64;
  auto t_progress = std::chrono::steady_clock::now();
  long long seen_last = -1;
  while (rc == MI355NDT_OK && !h->h_seq_flags[0] && enq < max_launches) {
    const long long seen = h->h_seq_flags[1];
    if (seen != seen_last) { seen_last = seen; t_progress = std::chrono::steady_clock::now(); }
    if (enq - seen >= depth) {
      // (a device that stops answering -- a faulted kernel -- must not leave the host spinning here)
      if (std::chrono::steady_clock::now() - t_progress > std::chrono::seconds(20)) { stuck = true; break; }
      std::this_thread::yield();
      continue;
    }
    k_seq_update<<<1, UPD_THREADS, 0, s>>>(h->d_seq, h->d_state, h->d_partials, h->rows_per_pair, h->pts_per_chunk, h->d_results, h->d_grid, h->d_src_cnt,
                                           h->d_stamps, h->d_seq_out, h->d_active_list, h->d_ctl + h->ctl_idx, h->d_grid_of, h->d_seq_flags,
                                           h->prm.step_size, h->prm.trans_epsilon, h->prm.max_iterations);
    rc = launch_sweep(h, sc, 1);
    enq++;
  }
  hipError_t e = hipEventRecord(ev[2], s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  h->prof = keep_prof;
  if (e != hipSuccess) { h->err = std::string("sequence run: ") + hipGetErrorString(e); return MI355NDT_ERR_HIP; }
  if (rc) return rc;
  HIPCHK(h, hipGetLastError());
  if (stuck || !h->h_seq_flags[0]) { h->err = stuck ? "sequence run: the device stopped making progress" : "sequence run did not finish within its launch budget"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipMemcpy(out_frames, h->d_seq_out, (size_t)n_frames * sizeof(mi355ndt_seq_frame), hipMemcpyDeviceToHost));
  if (out_results) HIPCHK(h, hipMemcpy(out_results, h->d_results, (size_t)n_frames * sizeof(mi355ndt_result), hipMemcpyDeviceToHost));
  if (stats) {
    float b_ms = 0, t_ms = 0;
    HIPCHK(h, hipEventElapsedTime(&b_ms, ev[0], ev[1]));
    HIPCHK(h, hipEventElapsedTime(&t_ms, ev[1], ev[2]));
    stats->upload_ms = upload_ms;
    stats->build_ms = b_ms;
    stats->track_ms = t_ms;
    stats->aligns = n_frames > 1 ? n_frames : 0;
    stats->update_launches = h->h_seq_flags[1];
  }
  return compute_enqueued(h);
}

int mi355ndt_sequence_run(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride,
                          const double* stamps, const mi355ndt_seq_params* policy,
                          mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results, mi355ndt_seq_stats* stats) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  NOT_EULER(h, "mi355ndt_sequence_run");
  size_t maxn = 0;
  int rc = sequence_args(h, n_frames, clouds, counts, stride, stamps, out_frames, (size_t)1 << 31, &maxn);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  const auto t_up0 = std::chrono::steady_clock::now();
  // every frame is a TARGET slot (its voxel grid is built: it may become a keyframe) and, through the same rows, the SOURCE of its own
  // align: one cloud buffer serves both sides
  rc = mi355ndt_batch_reserve(h, n_frames, maxn, 64);
  if (rc) return rc;
  rc = mi355ndt_batch_set_clouds(h, 0, n_frames, clouds, counts, nullptr, nullptr, stride, 0);
  if (rc) return rc;
  for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));     // (upload time is reported on its own)
  const auto t_up1 = std::chrono::steady_clock::now();
  return sequence_tracked(h, n_frames, stamps, policy, out_frames, out_results, stats, std::chrono::duration<double, std::milli>(t_up1 - t_up0).count());
}

// the same over RAW scans: the batch prefilter puts the frames into their slots (sized for the raw counts: a filtered cloud is no larger);
// outlier != NULL: the nodelet's third stage follows over the same slots (the frames are target slots; the run aliases them as sources)
int mi355ndt_sequence_run_raw_outliers(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride,
                                       const double* stamps, const mi355ndt_prefilter_params* pf, const mi355ndt_outlier_params* outlier,
                                       const mi355ndt_seq_params* policy, mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results,
                                       mi355ndt_seq_stats* stats, size_t* filtered_counts, double* prefilter_ms) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  NOT_EULER(h, "mi355ndt_sequence_run");
  size_t maxn = 0;
  int rc = sequence_args(h, n_frames, clouds, counts, stride, stamps, out_frames, (size_t)1 << 30, &maxn);
  if (rc) return rc;
  if (outlier) { rc = outlier_params_check(h, *outlier, "batch_remove_outliers"); if (rc) return rc; }
  HIPCHK(h, hipSetDevice(h->device));
  const auto t_up0 = std::chrono::steady_clock::now();
  rc = mi355ndt_batch_reserve(h, n_frames, maxn, 64);
  if (rc) return rc;
  std::vector<size_t> filtered((size_t)n_frames, 0);
  double kernels_ms = 0.0;
  rc = batch_prefilter_impl(h, 0, n_frames, clouds, counts, nullptr, nullptr, stride, pf, filtered.data(), nullptr, &kernels_ms);
  if (rc) { if (rc != MI355NDT_ERR_BAD_ARG && h->ev_compute) (void)compute_enqueued(h); return rc; }
  if (outlier) {
    double outlier_ms = 0.0;
    rc = batch_outliers_impl(h, 0, n_frames, 2, outlier, filtered.data(), nullptr, nullptr, nullptr, &outlier_ms);
    if (rc) { if (rc != MI355NDT_ERR_BAD_ARG && h->ev_compute) (void)compute_enqueued(h); return rc; }
    kernels_ms += outlier_ms;
  }
  const auto t_up1 = std::chrono::steady_clock::now();
  if (filtered_counts) std::copy(filtered.begin(), filtered.end(), filtered_counts);
  if (prefilter_ms) *prefilter_ms = kernels_ms;
  for (int k = 0; k < n_frames; k++)
    if (filtered[(size_t)k] == 0) { h->err = "sequence run: frame " + std::to_string(k) + " is empty after the prefilter"; return MI355NDT_ERR_BAD_ARG; }
  // staging and kernels alternate group by group inside the prefilter: what the host clock saw of it, less the kernels' own time, is the staging
  const double up_ms = std::max(0.0, std::chrono::duration<double, std::milli>(t_up1 - t_up0).count() - kernels_ms);
  return sequence_tracked(h, n_frames, stamps, policy, out_frames, out_results, stats, up_ms);
}

int mi355ndt_sequence_run_raw(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride,
                              const double* stamps, const mi355ndt_prefilter_params* pf, const mi355ndt_seq_params* policy,
                              mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results, mi355ndt_seq_stats* stats,
                              size_t* filtered_counts, double* prefilter_ms) {
  return mi355ndt_sequence_run_raw_outliers(h, n_frames, clouds, counts, stride, stamps, pf, nullptr, policy, out_frames, out_results, stats,
                                            filtered_counts, prefilter_ms);
}
