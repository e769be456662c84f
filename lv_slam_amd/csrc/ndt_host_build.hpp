// ndt_host_build.hpp -- the target build's host side: workspace, the one wait for the grid sizes (or the stream's plan instead), the kernel chain
// of ndt_build.hpp / ndt_segsort.hpp; ensure_grids, through which every surface that reads the grids asks for them.
#pragma once

// ---- target build -----------------------------------------------------------------------------
// `make`: what to build beside the base records (ndt_grid_state.hpp).  h->built is filled here, at the end, and nowhere else.
static int build_targets_impl(mi355ndt_handle* h, const GridExtras make) {
  if (h->n_pairs <= 0 || !h->d_tgt) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  { int rcu = uploads_before_compute(h); if (rcu) return rcu; }
  const int B = h->n_pairs;
  const size_t pitch = h->tgt_pitch;
  const size_t total = (size_t)B * pitch;
  hipStream_t s = h->stream;
  if (h->async_build && h->counts_preloaded) {
    h->up_tgt_cnt.clear();                          // stream mode: the counts came with the batch's one input copy (mi355ndt_stream_submit)
  } else if (h->up_tgt_cnt.size() != (size_t)B || !std::equal(h->up_tgt_cnt.begin(), h->up_tgt_cnt.end(), h->h_tgt_cnt.begin())) {
    HIPCHK(h, hipMemcpyAsync(h->d_tgt_cnt, h->h_tgt_cnt.data(), B * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));   // h_tgt_cnt is pageable
    h->up_tgt_cnt.assign(h->h_tgt_cnt.begin(), h->h_tgt_cnt.begin() + B);   // exactly what the device now holds
  }

  // workspace
  HIPCHK(h, h->d_keys_a.reserve(total)); HIPCHK(h, h->d_keys_b.reserve(total));
  HIPCHK(h, h->d_vals_a.reserve(total)); HIPCHK(h, h->d_vals_b.reserve(total));
  const int minpts = h->prm.min_points_per_voxel;
  const size_t rpp = pitch / (size_t)minpts + 1;
  if (rpp > ((size_t)1 << ID_BITS)) { h->err = "target too large: voxel ids would not fit the sweep's queue entries"; return MI355NDT_ERR_BAD_ARG; }
  if ((size_t)B * rpp > h->d_recs.cap || rpp != h->recs_per_pair) {
    const size_t need = (size_t)B * rpp;
    h->recs_per_pair = 0;                         // (until the whole group exists again: a failure half way is retried by the next build)
    HIPCHK(h, h->d_recs.realloc_exact(need)); HIPCHK(h, h->d_vox_idx.realloc_exact(need)); HIPCHK(h, h->d_vox_n.realloc_exact(need));
    HIPCHK(h, h->d_seg_start.realloc_exact(need)); HIPCHK(h, h->d_sums.realloc_exact(need * 9)); HIPCHK(h, h->d_cent.realloc_exact(need * 3));
    h->recs_per_pair = rpp;
  }
  h->ev_last_fresh = false;
  const bool build_events = h->prof && !(h->build_stamped && h->async_build);   // (the stream's builds are stamped by the kernels around them)
  if (build_events) HIPCHK(h, ev_begin(h, h->ev_build));
  const int gx = (int)((pitch + 255) / 256);
  h->built.valid = false;                         // (the kernels below overwrite what it describes: an error exit leaves no valid-looking grids)
  if (!h->word_off_cleared) HIPCHK(h, hipMemsetAsync(h->d_word_off, 0, (2 + 6 * (size_t)h->cap_pairs) * sizeof(unsigned), s));   // (stream mode: k_stream_inputs did)
  h->word_off_cleared = false;
  k_minmax<<<dim3(std::max(1, std::min((gx + 3) / 4 / MM_ILP, 64)), B), 256, 0, s>>>(h->d_tgt, pitch, h->d_tgt_cnt, h->d_minmax);
  k_griddesc<<<(B + 63) / 64, 64, 0, s>>>(h->d_minmax, h->d_grid, h->d_nwords, h->prm.resolution, B, (unsigned)rpp);
  k_word_offsets<<<1, 1024, 0, s>>>(h->d_grid, h->d_nwords, B, h->d_word_off);   // d_word_off[0] = total words, [1] = largest grid
  size_t total_words;
  int cb;
  const bool planned = h->async_build && h->plan_cb > 0 && h->plan_words > 0 && h->plan_words <= h->d_words.cap && h->d_bstat;
  if (planned) {
    // no wait: the plan's key width and pool size, checked on the device (a batch that does not fit loses its grids and is flagged)
    k_build_check<<<(B + 255) / 256, 256, 0, s>>>(h->d_word_off, h->d_grid, h->d_nwords, B, (unsigned)std::min(h->plan_words, (size_t)0xFFFFFFFFu), h->plan_cb, h->d_bstat + 1);
    total_words = h->plan_words;
    cb = h->plan_cb;
  } else {
    HIPCHK(h, hipMemcpyAsync(h->h_pin_u, h->d_word_off, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));           // total bitmap words -> size the pool; largest grid -> key width
    total_words = h->h_pin_u[0];
    cb = std::max(1, ceil_log2(h->h_pin_u[1] + 1u));   // cell field: every cell index + the all-ones "not binned" value
    if (h->async_build) cb = std::max(cb, h->plan_cb);        // (a wider field sorts the same order: the plan only ever grows)
    if (h->d_bstat) HIPCHK(h, hipMemsetAsync(h->d_bstat + 3, 0, sizeof(unsigned), s));
  }
  if (total_words > h->d_words.cap) HIPCHK(h, h->d_words.reserve(std::max(total_words, (size_t)1024)));
  if (total_words) HIPCHK(h, hipMemsetAsync(h->d_words, 0, total_words * sizeof(BitWord), s));
  const bool want_cent = make.cent, fast_recs = make.recs_fast, want_kdw = make.kdw;
  if (make.icov64) HIPCHK(h, h->d_icov64.reserve(h->d_recs.cap * 9));
  if (fast_recs) HIPCHK(h, h->d_recs_fast.reserve(h->d_recs.cap));
  if (want_kdw) HIPCHK(h, h->d_kdw.reserve(h->d_recs.cap));
  if (make.leaf_class) HIPCHK(h, h->d_leaf_class.reserve(h->d_recs.cap));
  {
    unsigned *ka = h->d_keys_a, *kb = h->d_keys_b;
    // stable sort by cell inside every target's segment (ndt_segsort.hpp): rs_plan(cb) passes, result in kb / d_vals_b
    const RsPlan plan = rs_plan(cb);
    const int npass = plan.passes;
    const int tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
    const size_t rs_need = ((size_t)B * tiles) << RS_MAX_BITS;
    HIPCHK(h, h->d_rs_hist.reserve(rs_need)); HIPCHK(h, h->d_rs_offs.reserve(rs_need));
    unsigned *kin = (npass & 1) ? ka : kb, *kout = (npass & 1) ? kb : ka;      // an odd number of hops must end in kb
    unsigned *vin = (npass & 1) ? h->d_vals_a : h->d_vals_b, *vout = (npass & 1) ? h->d_vals_b : h->d_vals_a;
    // (no key kernel: the first pass's histogram computes the cell indices from the points and writes them, ndt_segsort.hpp)
    const RsPoints points = {h->d_tgt, h->d_tgt_cnt, h->d_grid, cb, kin};
    if (!rs_disjoint(kin, vin, kout, vout, total)) { h->err = "target build: the sort's two buffer pairs overlap"; return MI355NDT_ERR_STATE; }
    for (int p = 0; p < npass; p++) {
      rs_pass(s, plan.bits, kin, vin, kout, vout, pitch, p * plan.bits, h->d_rs_hist, h->d_rs_offs, tiles, B, p == 0, p == 0 ? &points : nullptr);
      std::swap(kin, kout); std::swap(vin, vout);
    }
    // k_mark leaves the leaves' run starts in per-wave slices; k_rank strings them together by voxel id (d_seg_start)
    const unsigned nsl = ls_slices(pitch), scap = ls_slice_cap(minpts);
    HIPCHK(h, h->d_heads.reserve((size_t)B * nsl * scap));
    HIPCHK(h, h->d_head_cnt.reserve((size_t)B * nsl));
    k_mark<unsigned><<<dim3((nsl + 3) / 4, B), 256, 0, s>>>(kb, pitch, h->d_grid, h->d_words, h->d_heads, h->d_head_cnt, nsl, scap, minpts, cb);
    k_rank<<<B, RANK_THREADS, 0, s>>>(h->d_grid, h->d_words, h->d_heads, h->d_head_cnt, nsl, scap, h->d_seg_start);
    // leaf-sum workgroups per target: 64 keeps ~4 targets (3 MB of points) in flight per XCD, inside its 4 MB L2
    const int lb = std::max(1, std::min((int)((rpp + LS_WAVES - 1) / LS_WAVES), 64));
    auto leafsum = [&](auto kern, const unsigned* vals) {
      kern<<<xcd_grid(lb, B), 64 * LS_WAVES, 0, s>>>(h->d_tgt, pitch, kb, vals, h->d_grid, h->d_seg_start, h->d_sums, h->d_vox_idx, h->d_vox_n, cb, h->d_cent, lb, B);
    };
    if (fast_recs && !want_cent && !h->leaf_sorted) {      // tolerance arithmetic: the leaf sums as a tree (ndt_build.hpp)
      k_leafsum_tree<<<xcd_grid(lb, B), 64 * LS_WAVES, 0, s>>>(h->d_tgt, pitch, kb, h->d_vals_b, h->d_grid, h->d_seg_start, h->d_sums, h->d_vox_idx, h->d_vox_n, cb, lb, B);
    } else if (h->leaf_sorted) {
      // the sorted order as 16-byte points first (one streaming gather), then leaf sums that read them contiguously
      HIPCHK(h, h->d_sorted.reserve(total));
      const int gb = std::max(1, std::min((int)((pitch + 256 * RUN_ILP - 1) / (256 * RUN_ILP)), 64));
      k_sorted_points<<<xcd_grid(gb, B), 256, 0, s>>>(h->d_tgt, pitch, h->d_vals_b, h->d_sorted, gb, B);
      leafsum(want_cent ? k_leafsum<unsigned, true, true> : k_leafsum<unsigned, false, true>, reinterpret_cast<const unsigned*>(h->d_sorted.p));
    } else leafsum(want_cent ? k_leafsum<unsigned, true> : k_leafsum<unsigned, false>, h->d_vals_b);
  }
  k_voxels<<<dim3((unsigned)((rpp + 255) / 256), B), 256, 0, s>>>(h->d_grid, h->d_sums, h->d_recs, h->d_vox_n,
                                                                  h->prm.min_covar_eigvalue_mult, h->prm.variant == MI355NDT_VARIANT_PCA,
                                                                  make.icov64 ? h->d_icov64 : nullptr, want_kdw ? h->d_kdw : nullptr, fast_recs ? h->d_recs_fast : nullptr,
                                                                  make.leaf_class ? h->d_leaf_class.p : nullptr);
  HIPCHK(h, hipGetLastError());
  if (h->prof) {
    if (build_events) HIPCHK(h, ev_end(h, h->ev_build));
    double pts = 0;
    for (int b = 0; b < B; b++) pts += h->h_tgt_cnt[b];
    // B_build: minmax 12 + binning 12 + key write 12 + sort r/w + grouped gather 16 per point (+ records)
    h->P.build_alg_bytes += pts * (12 + 12 + 4 + 16);
  }
  h->built = GridsBuilt{true, make, h->prm.resolution, cb, total_words, false};
  return compute_enqueued(h);                     // asynchronous: a later upload into these rows has to wait for the kernels above
}

static int build_targets(mi355ndt_handle* h, const GridExtras make) {
  NOT_IN_STREAM(h);
  const int rc = build_targets_impl(h, make);
  // an error exit may leave kernels queued that still read the cloud rows: later uploads have to wait for them all the same
  if (rc != MI355NDT_OK && h->ev_compute) (void)compute_enqueued(h);
  return rc;
}
int mi355ndt_batch_build_targets(mi355ndt_handle* h) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  return build_targets(h, eff_extras(h));
}

static int ensure_grids(mi355ndt_handle* h, GridWant want) {
  HIPCHK(h, hipSetDevice(h->device));             // the prologue of every call that reads the grids: the engine's device, the uploads so far
  { int rcu = uploads_before_compute(h); if (rcu) return rcu; }   // in front of the compute stream (the cloud rows are read as well)
  const GridExtras make = eff_extras(h, want == GRIDS_LIVE);
  return grids_serve(h->built, want == GRIDS_ANY ? GridExtras{} : make) ? (int)MI355NDT_OK : build_targets(h, make);
}
