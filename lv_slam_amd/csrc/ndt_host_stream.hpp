// ndt_host_stream.hpp -- stream mode (mi355ndt_stream_*): session begin / end, the persistent launch per submitted batch, the one synchronous path
// of a context (stream_run_sync), collect, pose records.
#pragma once

// ---- stream mode ----------------------------------------------------------------------------------------------------------
// (include/mi355_ndt.h: mi355ndt_stream_*; kernels: ndt_async.hpp.  Replaces a run of batch_bind_device + batch_build_targets +
//  batch_align triples for batches that arrive one after the other -- scan_matching_odom_nodelet.cpp:144-183 is a stream of frames.)
// What a submit puts on the stream: ONE input copy, the build's kernels and two fills, the prepare kernel, the persistent launch, the
// status kernel.  No device-to-host copy, no event: result records and launch status land in mapped host memory.  (The first form of
// this path issued ~17 copies and fills per batch; at ~20 us of stream time each they cost more than the tail they removed.)
// The stream's fixed row geometry, the same for every batch of a context (a pair's rows do not depend on it); a synchronous align
// re-computes its own (prep_align_ws), so it is put back afterwards.  stream_partials: the d_partials every context holds for it.
static void stream_geometry(const StreamState& ss, mi355ndt_handle* e) {
  e->chunks_per_pair = ss.items / QUARTERS; e->rows_per_pair = e->items_per_pair = ss.items; e->pts_per_chunk = CHUNK_PTS; e->fine_it = 0;
}
static size_t stream_partials(const StreamState& ss) { return (size_t)ss.max_pairs * ss.items * NACC; }
// A build of context engine `e` that waited for its sizes teaches the stream its plan: key width and pool words the later builds run
// against without waiting (with headroom: scans of one drive vary by a few per cent).  The plan only ever grows.
static void stream_learn_plan(StreamState& ss, const mi355ndt_handle* e) {
  ss.plan_cb = std::max(ss.plan_cb, e->built.cb);
  ss.plan_words = std::max(ss.plan_words, e->built.total_words + e->built.total_words / 4 + 1024);
}
int mi355ndt_stream_end(mi355ndt_handle* h) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!h->ss) return MI355NDT_OK;
  (void)hipSetDevice(h->device);
  StreamState& ss = *h->ss;
  if (ss.build_stream) (void)hipStreamSynchronize(ss.build_stream);
  (void)hipStreamSynchronize(h->stream);
  // the contexts' build timings and byte counts belong to this handle's profile
  for (int c = 0; c < ss.nctx; c++) {
    mi355ndt_handle* e = ss.ctx[c].e.get();
    if (!e) continue;
    ev_collect(e, e->ev_sweep, h->P.sweep_ms, h->P.sweep_launches);
    ev_collect(e, e->ev_update, h->P.update_ms, h->P.update_launches);
    ev_collect(e, e->ev_build, h->P.build_ms, h->P.build_launches);
    h->P.build_alg_bytes += e->P.build_alg_bytes; e->P.build_alg_bytes = 0;
  }
  h->ss.reset();                                  // (the contexts' engines, the session's buffers, events and build stream, a pending pose-record request)
  return MI355NDT_OK;
}

int mi355ndt_stream_begin(mi355ndt_handle* h, int n_contexts, int max_pairs, size_t max_tgt, size_t max_src) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (n_contexts < 2 || n_contexts > ASYNC_MAX_CTX || max_pairs < 1 || max_pairs > MAX_PAIRS || max_pairs >= (1 << ASYNC_CTX_SHIFT) ||
      max_tgt == 0 || max_src == 0 || max_tgt >= (1u << 31) || max_src >= (1u << 31)) return MI355NDT_ERR_BAD_ARG;
  if (h->ss) return MI355NDT_ERR_STATE;
  NOT_EULER(h, "mi355ndt_stream_begin");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::unique_ptr<StreamState> session(new StreamState());   // (a failure below releases whatever was created before it)
  StreamState& ss = *session;
  ss.nctx = n_contexts; ss.max_pairs = max_pairs; ss.max_tgt = max_tgt; ss.max_src = max_src;
  ss.items = std::max(1, (int)((max_src + CHUNK_PTS - 1) / CHUNK_PTS)) * QUARTERS;
  ss.sync_only = !async_served(h);
  // the grids a streamed launch reads are the contexts' (built at prm.resolution); whatever single-registration grid the parent still holds
  // -- possibly one a setResolution without a source left at another leaf size (ndt_omp.h:126-136) -- is no part of the stream
  h->built = GridsBuilt{};
  SweepConst sc;
  make_sweep_const(h, sc);
  // (the session is sized for the geometry every configuration has; whether a launch of exact ndt_omp / DIRECT7 runs the lean body on 768 slots
  //  instead is decided launch by launch, from the batch that launch starts: stream_launch)
  const int slots = launch_slots(h, sc, fast_served(h));
  {
    const int iu = ss.items / (sc.K == 1 ? ASYNC_CLAIM(1) : sc.K == 7 ? 2 : 1);   // positions per ticket (DIRECT1: ndt_async.hpp; stream_launch: two DIRECT7 items per claim when pairs are handed over)
    const int waves = slots * WAVES;
    // automatic: four sweeps' worth of positions per resident wave -- `tools/gpu_job.sh thresh_sweep`: config 5 gains up to T = 32-64 (DIRECT7 19.1 / 19.4 / 19.5 k,
    // DIRECT1 39.4 / 40.1 / 40.9 / 41.1 k registrations/s at T = 8 / 16 / 32 / 64), the 65,536-point configurations do not care -- capped at a quarter of the batch (stream_launch)
    int t = h->s_thresh_opt >= 0 ? h->s_thresh_opt : 4 * ((waves + iu - 1) / std::max(1, iu));
    const char* env = std::getenv("MI355NDT_STREAM_THRESH");
    if (env) t = std::atoi(env);
    ss.thresh = std::max(0, std::min(t, ASYNC_MAX_CARRY));
    ss.thresh_given = h->s_thresh_opt >= 0 || env;
  }
  {
    // MI355NDT_STREAM_RESERVE (workgroups, rounded to a multiple of 8; 0 = the build runs between the launches, on the same stream).  Defaults
    // (tools/reserve_sweep_*.sh, reserve_matrix.sh, reserve_resweep*.sh; a launch's time grows with the slots it gives away, 512 / (512 - r), in every search:
    // what is won is the build's time):
    //  * DIRECT1: 128 for clouds of up to 98,304 points, 96 beyond.  Its launches wait for their point stream more than they compute (VALU busy 0.4-0.6) and
    //    are short enough for the build to be 30 % of a step: nodelet configuration (1 m, 65,536 points) r = 0 / 64 / 96 / 112 / 128 / 160: 112.1 / 117.3 /
    //    122.1 / 120.1 / 124.7 / 116.8 k registrations/s; config 5's clouds (0.5 m, 131,072 points) 42.3 / - / 44.5 / - / 43.0 k; 64-pair batches 65.4 -> 96.6 k.
    //  * ndt_omp / DIRECT7 (the headline's configuration): 64 = eight slots per XCD.  The launch is VALU-bound, so the slots are paid for in full
    //    (3.95 -> 4.41 ms) -- but the whole 0.70 ms build disappears under it: 57.3 -> 59.7 k and 55.7 -> 59.2 k on two boxes (r = 0 / 16 / 32 / 48 /
    //    64 / 80 / 96 / 128: 55.7 / 56.3 / 57.4 / 56.9 / 59.2 / 57.9 / 56.1 / 53.4 k); the tolerance arithmetic +2 % (90.3 -> 92.3 k).
    //    The smaller the batch, the more it is worth (a small build is a chain of short kernels, not throughput): 64 pairs 41.3 -> 50.6 k; at 1,536 pairs
    //    per batch the build no longer fits under its launch: exact +-0, tolerance arithmetic -6 % (DIRECT1 still +4 %) -- so only for batches up to
    //    768 x 65,536 target points.
    //    The lean launch (three waves per SIMD, 768 slots, a slot = a third of a CU; chosen per launch: stream_launch): 96 = the same eighth of the GPU.  Swept on one box with
    //    plain bench.py runs (docs/experiments.md 10o), r = 0 / 32 / 48 / 64 / 80 / 96 / 112 / 128 / 160: 64.0 / 65.2 / 64.6 / 67.1 / 66.9 / 68.4 / 68.4 /
    //    68.4 / 66.9 k against 64.9 k for the two-wave launch at its 64 -- a plateau from 96 to 128, of which 96 leaves the launch the most slots.  Every
    //    kernel of the build has to fit a third of a CU for that: k_rank (ndt_build.hpp) is an eight-wave block since.
    //  * ndt_pca / DIRECT7: 32 (same bound on the batch).  Until the build was made to start BEHIND the launch's prepare kernel (stream_submit) its first kernels
    //    raced the launch's own start and r >= 64 cost a third of the rate; since then config 5 (0.5 m, 128 x 131,072) r = 0 / 16 / 32 / 48 / 64 / 96: 19.1 /
    //    19.3 / 20.0 / 19.6 / 19.8 / 18.8 k, 271 x 65,536 at 1 m 34.9 -> 35.3 k, 64-pair batches 31.7 -> 35.3 k.
    //  * Everything else (DIRECT26, KDTREE): 0.
    const bool small_batch = (unsigned long long)max_pairs * (unsigned long long)max_tgt <= 768ull * 65536ull;
    int r = sc.K == 1 ? (max_tgt <= 98304 ? 128 : 96) : ((sc.K == 7 && small_batch) ? (sc.pca ? 32 : 64) : 0);
    if (const char* e = std::getenv("MI355NDT_STREAM_RESERVE")) { r = std::atoi(e); ss.reserve_given = true; }
    if (h->s_reserve_opt >= 0) { r = h->s_reserve_opt; ss.reserve_given = true; }
    r = std::max(0, std::min(r, slots / 2)) & ~7;
    if (n_contexts < 3) r = 0;                       // (the overlapped build needs its context free one launch earlier: at least three contexts)
    ss.reserve_wg = r;
    ss.launch_slots = std::max(8, slots - r);
    ss.last_reserve = r; ss.last_slots = ss.launch_slots;       // (what the profile reports until the first launch says what it took)
  }
  ss.ring_cap = async_ring_cap(h, (long long)max_pairs + ASYNC_MAX_CARRY);
  if (ss.ring_cap == 0) ss.sync_only = true;
  if (ss.d_stat.realloc_exact(ASYNC_MAX_CTX) != hipSuccess ||
      hipMemsetAsync(ss.d_stat, 0, ASYNC_MAX_CTX * sizeof(CtxStat), h->stream) != hipSuccess) return MI355NDT_ERR_HIP;
  for (int c = 0; c < n_contexts; c++) {
    StreamCtx& S = ss.ctx[c];
    mi355ndt_handle* e = nullptr;
    int rc = mi355ndt_create(&h->prm, h->device, &e);
    S.e.reset(e);
    if (rc) return rc;
    if (ss.reserve_wg > 0 && !ss.build_stream) {
      if (ss.build_stream.create() != hipSuccess) return MI355NDT_ERR_HIP;
      for (auto& ev : ss.ev_built) if (ev.create() != hipSuccess) return MI355NDT_ERR_HIP;
      for (auto& ev : ss.ev_launched) if (ev.create() != hipSuccess) return MI355NDT_ERR_HIP;
      for (auto& ev : ss.ev_prepared) if (ev.create() != hipSuccess) return MI355NDT_ERR_HIP;
      if (const char* pf = std::getenv("MI355NDT_STREAM_PREP_FIRST")) ss.prep_first = std::atoi(pf) != 0;
    }
    rc = mi355ndt_set_stream(e, ss.reserve_wg > 0 ? ss.build_stream : h->stream);
    if (rc) return rc;
    e->sweep_waves = h->sweep_waves; e->f32_sum_order = h->f32_sum_order; e->arith = h->arith; e->async_align = h->async_align; e->dyn_shift = h->dyn_shift; e->score_only_last = h->score_only_last;
    e->async_build = true;
    e->ev_pool_target = 128;
    rc = ensure_pair_arrays(e, max_pairs);          // every per-pair array at its final size: no allocation, no wait inside submit
    if (rc) { h->err = e->err; return rc; }
    // the input block: [target counts | source counts | guesses]
    static_assert(sizeof(float) == sizeof(int), "the input block holds ints and floats");
    const size_t in_words = (size_t)max_pairs * (2 + 16);
    if (S.d_in.realloc_exact(in_words) != hipSuccess || S.h_in.realloc_exact(in_words, hipHostMallocMapped) != hipSuccess ||
        !(S.h_in_dev = (unsigned*)S.h_in.dev()) ||
        S.h_res.realloc_exact(max_pairs, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        !(S.d_res_map = S.h_res.dev())) { h->err = "stream_begin: allocation failed"; return MI355NDT_ERR_HIP; }
    e->d_tgt_cnt = S.d_in; e->d_src_cnt = S.d_in + max_pairs; e->d_guess = (float*)(S.d_in + 2 * (size_t)max_pairs);
    e->d_bstat = reinterpret_cast<unsigned*>(ss.d_stat + c);
    if (e->d_partials.reserve(stream_partials(ss)) != hipSuccess || e->d_arrived.reserve((size_t)max_pairs * ASYNC_ARR_STRIDE) != hipSuccess)
      { h->err = "stream_begin: allocation failed"; return MI355NDT_ERR_HIP; }
    if (h->prof) (void)mi355ndt_profile_enable(e, 1);
  }
  if (ss.d_ctl.realloc_exact(2) != hipSuccess || hipMemsetAsync(ss.d_ctl, 0, 2 * sizeof(AsyncCtl), h->stream) != hipSuccess ||
      ss.h_status.realloc_exact(StreamState::EV, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      !(ss.d_status = ss.h_status.dev())) return MI355NDT_ERR_HIP;
  memset((void*)ss.h_status.p, 0, StreamState::EV * sizeof(StreamStatus));
  if (h->d_atab.reserve(1) != hipSuccess) return MI355NDT_ERR_HIP;
  if (!ss.sync_only && ss.d_ring.realloc_exact((size_t)8 * ss.ring_cap) != hipSuccess) { (void)hipGetLastError(); ss.sync_only = true; }
  if (ss.build_stream) HIPCHK(h, hipStreamSynchronize(ss.build_stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ss = std::move(session);
  return MI355NDT_OK;
}

// one persistent launch of the stream: the pairs the previous launch suspended + the `n_new` pairs of context `new_ci` (-1: a flush --
// nothing new, everything runs to its end), then the status kernel (launch outcome + every context's counters -> mapped host memory)
static int stream_launch(mi355ndt_handle* h, int new_ci, int n_new) {
  StreamState& ss = *h->ss;
  hipStream_t s = h->stream;
  SweepConst sc;
  make_sweep_const(h, sc);
  AsyncLaunch L;
  memset(&L.tab, 0, sizeof L.tab);
  const bool flush = new_ci < 0;
  for (int c = 0; c < ss.nctx; c++) {
    mi355ndt_handle* e = ss.ctx[c].e.get();
    if (!e->d_src) continue;                         // never bound: no ticket can name it
    fill_async_ctx(e, L.tab.c[c]);
    L.tab.c[c].results = ss.ctx[c].d_res_map;
    L.tab.c[c].n_done = &ss.d_stat[c].done;
    L.tab.c[c].pose = ss.ctx[c].busy ? ss.ctx[c].d_pose : nullptr; L.tab.c[c].pose_base = ss.ctx[c].pose_base; L.tab.c[c].pose_stride = ss.ctx[c].pose_stride;
    // The context the NEXT submit recycles must be finished by this launch; the others may hand their last pairs over.  With three or more
    // contexts the context after that one must finish too: its batch is then complete one launch BEFORE the submit that recycles it, so the
    // host collects it and enqueues the next build while a launch is still running -- otherwise every collect returns at the very end of a
    // launch and the GPU idles for as long as the host takes to notice, collect and enqueue (~0.1-0.2 ms per batch, measured as the
    // difference between a streamed step and its kernels).  (The build under the launch -- s_reserve_wg -- needs the same.)
    const int ahead = (ss.reserve_wg > 0 || ss.nctx >= 3) ? 2 : 1;
    bool mf = flush;
    for (int a = 1; a <= ahead; a++) mf = mf || c == (new_ci + a) % ss.nctx;
    L.tab.c[c].must_finish = mf ? 1 : 0;
  }
  const long long j = ss.launches;
  L.new_ci = flush ? 0 : new_ci; L.n_new = flush ? 0 : n_new;
  if (!flush) {
    mi355ndt_handle* e = ss.ctx[new_ci].e.get();
    L.st_new = e->d_state; L.guess_new = e->d_guess; L.src_cnt_new = e->d_src_cnt; L.gd_new = e->d_grid; L.arrived_new = e->d_arrived;
    L.active_list = e->d_active_list; L.sweep_ctl = nullptr; L.done_new = &ss.d_stat[new_ci].done;
    L.pose_new = ss.ctx[new_ci].d_pose; L.pose_cap = ss.ctx[new_ci].pose_cap;
  }
  L.tab_dev = h->d_atab; L.ring = ss.d_ring; L.ring_cap = ss.ring_cap;
  L.ctl = ss.d_ctl + (j & 1); L.prev = ss.drop_carry ? nullptr : ss.d_ctl + ((j + 1) & 1);
  // (the automatic threshold never hands over more than a quarter of the batch: a batch too small to fill the GPU has no bulk to hide stragglers under)
  L.items_per_pair = ss.items; L.stop_thresh = flush ? 0 : (ss.thresh_given ? ss.thresh : std::min(ss.thresh, n_new / 4)); L.debug_abort_pos = h->debug_abort_pos; L.debug_ring_mask = h->debug_ring_mask;
  // Two or three waves per SIMD, launch by launch: the batch this launch starts says (its largest target; a flush runs what the launch before
  // it ran).  A lean launch has 768 slots, a third of a CU each: a reserve the caller named is taken as named, the default becomes LEAN_RESERVE_WG
  // -- the same eighth of the GPU as the two-wave launch's 64 -- wherever the two-wave default reserves at all.
  if (!flush) {
    const mi355ndt_handle* e = ss.ctx[new_ci].e.get();
    const int tgt_max = *std::max_element(e->h_tgt_cnt.begin(), e->h_tgt_cnt.begin() + n_new);
    ss.lean = async_lean(h, sc, sweep_ord(h, sc), tgt_max > 0 ? (size_t)tgt_max : ss.max_tgt);
  }
  L.lean = ss.lean;
  L.reserve_wg = flush ? 0 : ss.reserve_wg;
  if (L.lean && !flush && !ss.reserve_given && ss.reserve_wg > 0) L.reserve_wg = LEAN_RESERVE_WG;
  if (L.lean) L.reserve_wg = std::min(L.reserve_wg, launch_slots(h, sc, false, true) / 2) & ~7;
  L.ev_prepared = (ss.reserve_wg > 0 && ss.prep_first) ? ss.ev_prepared[j % StreamState::EV] : nullptr;
  // two DIRECT7 items per claim halve the hand-overs between items (+1.4-2 %); the coarser positions lengthen a launch's own tail, so only
  // where the tail is handed on (docs/experiments.md 10d)
  L.claim_items = (sc.K == 7 && L.stop_thresh > 0) ? 2 : 1;
  h->ev_last_fresh = false;                          // (the contexts' builds sit between two launches on this stream)
  if (!flush && ss.reserve_wg > 0) HIPCHK(h, hipStreamWaitEvent(s, ss.ev_built[new_ci], 0));   // this batch's grids (built on the other stream)
  L.stamp_end = (!flush && h->prof) ? &ss.d_status[j % StreamState::EV].build_t1 : nullptr;
  int rc = launch_async(h, sc, L);
  if (rc) return rc;
  ss.drop_carry = false;
  if (!flush) { ss.last_reserve = L.reserve_wg; ss.last_slots = h->last_async_grid; }
  const int slot = (int)(j % StreamState::EV);
  k_stream_status<<<1, 64, 0, s>>>(L.ctl, ss.d_stat, reinterpret_cast<volatile unsigned*>(ss.d_status + slot), (unsigned)(j + 1));
  HIPCHK(h, hipGetLastError());
  if (ss.reserve_wg > 0) HIPCHK(h, hipEventRecord(ss.ev_launched[slot], s));
  ss.launches++;
  h->P.stream_launches++;
  return MI355NDT_OK;
}

// wait until launch j has reported (its status slot carries sequence number j + 1): the host polls mapped memory
static int stream_wait_launch(mi355ndt_handle* h, long long j) {
  StreamState& ss = *h->ss;
  volatile StreamStatus* st = ss.h_status + (j % StreamState::EV);
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0; st->seq != (unsigned)(j + 1); spins++) {
    if ((spins & 1023) == 1023) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) { h->err = "stream: the device stopped reporting"; return MI355NDT_ERR_STATE; }
      std::this_thread::yield();
    } else cpu_relax();
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for (; ss.counted <= j; ss.counted++) {       // (launches finish in order)
    volatile StreamStatus* c = ss.h_status + (ss.counted % StreamState::EV);
    h->P.stream_carried += c->susp;
    const unsigned long long b0 = c->build_t0, b1 = c->build_t1;
    if (b0 && b1 > b0) { h->P.build_ms += (double)(b1 - b0) * 1e-5; h->P.build_launches++; }   // wall_clock64: 100 MHz
    c->build_t0 = 0; c->build_t1 = 0;
  }
  return MI355NDT_OK;
}

// The ONE synchronous path of a context: whatever is in flight drains, the context's engine builds and aligns its batch here and now (results
// into S.h_res), and what the stream keeps per context is put back -- the plan learns from the build that just waited for its sizes, the
// engine returns to the stream's row geometry.  Taken by a session the one-launch align does not serve, after a launch that could not be
// made, and by collect for a batch whose launch gave up or whose build exceeded the plan.  (A sync_only session has idle streams here and
// never reads the plan or the geometry again: for it those steps change nothing.)
static int stream_run_sync(mi355ndt_handle* h, StreamCtx& S) {
  StreamState& ss = *h->ss;
  mi355ndt_handle* e = S.e.get();
  if (ss.build_stream) HIPCHK(h, hipStreamSynchronize(ss.build_stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  e->async_build = false; e->counts_preloaded = false;
  e->up_tgt_cnt.clear(); e->up_src_cnt.clear();
  int rc = mi355ndt_batch_build_targets(e);
  if (rc == MI355NDT_OK) rc = mi355ndt_batch_align(e, S.guesses.data(), S.h_res);
  e->async_build = true;
  if (rc) { h->err = e->err; return rc; }
  stream_learn_plan(ss, e);
  stream_geometry(ss, e);
  if (e->d_partials.reserve(stream_partials(ss)) != hipSuccess) return MI355NDT_ERR_HIP;
  return MI355NDT_OK;
}

int mi355ndt_stream_submit(mi355ndt_handle* h, int n_pairs, const float* d_t, const int* tc, size_t tp, const float* d_s, const int* scnt, size_t sp,
                           const float* guesses, long long* batch_id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!h->ss) return MI355NDT_ERR_STATE;
  StreamState& ss = *h->ss;
  if (n_pairs < 1 || n_pairs > ss.max_pairs || !guesses || !batch_id || !tc || !scnt) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const long long id = ss.next_id;
  const int ci = (int)(id % ss.nctx);
  StreamCtx& S = ss.ctx[ci];
  if (S.busy) { h->err = "stream_submit: collect batch " + std::to_string(S.batch_id) + " first (its context is the one this batch needs)"; return MI355NDT_ERR_STATE; }
  mi355ndt_handle* e = S.e.get();
  for (int b = 0; b < n_pairs; b++) if ((size_t)scnt[b] > (size_t)(ss.items / QUARTERS) * CHUNK_PTS) return MI355NDT_ERR_BAD_ARG;   // more source points than stream_begin was told
  int rc = mi355ndt_batch_bind_device(e, n_pairs, d_t, tc, tp, d_s, scnt, sp);
  if (rc) { h->err = e->err; return rc; }
  e->prm = h->prm;
  S.batch_id = id; S.n_pairs = n_pairs; S.redo = false; S.done_sync = false; S.launch = -1;
  S.guesses.assign(guesses, guesses + (size_t)n_pairs * 16);
  S.d_pose = (PoseRecord*)ss.pose_next; S.pose_cap = (int)ss.pose_cap_next; S.pose_base = ss.pose_base_next; S.pose_stride = ss.pose_stride_next;
  ss.pose_next = nullptr; ss.pose_cap_next = 0;
  if (S.d_pose && (size_t)n_pairs > (size_t)S.pose_cap) return MI355NDT_ERR_BAD_ARG;
  if (ss.sync_only) {                              // a configuration the one-launch align does not serve: processed here and now
    rc = stream_run_sync(h, S);
    if (rc) return rc;
    S.done_sync = true; S.busy = true;
    *batch_id = id; ss.next_id++;
    return MI355NDT_OK;
  }
  // the batch's small inputs in one copy: point counts of both sides, guesses
  memcpy(S.h_in, tc, (size_t)n_pairs * sizeof(int));
  memcpy(S.h_in + ss.max_pairs, scnt, (size_t)n_pairs * sizeof(int));
  memcpy(S.h_in + 2 * (size_t)ss.max_pairs, guesses, (size_t)n_pairs * 16 * sizeof(float));
  // this context's previous batch was finished by the launch before the last one (must_finish): the build may start when that launch has ended -- and
  // a moment later still, when the LAST launch's prepare kernel is through (it follows that end on the stream): the build's first kernels stream the
  // whole batch through HBM and would otherwise run against the one short kernel every launch waits for (k_async_prepare: 50 us beside k_minmax, 17 alone)
  if (ss.reserve_wg > 0 && ss.prep_first && ss.launches >= 1)
    HIPCHK(h, hipStreamWaitEvent(e->stream, ss.ev_prepared[(ss.launches - 1) % StreamState::EV], 0));
  else if (ss.reserve_wg > 0 && ss.launches >= 2)
    HIPCHK(h, hipStreamWaitEvent(e->stream, ss.ev_launched[(ss.launches - 2) % StreamState::EV], 0));
  // (one workgroup reads the block from mapped host memory and clears the build's word block: no copy, no fill -- k_stream_inputs)
  k_stream_inputs<<<1, 1024, 0, e->stream>>>(S.h_in_dev, reinterpret_cast<unsigned*>(S.d_in.p), (unsigned)(2 * (size_t)ss.max_pairs + (size_t)n_pairs * 16),
                                            e->d_word_off, (unsigned)(2 + 6 * (size_t)e->cap_pairs),
                                            h->prof ? &ss.d_status[ss.launches % StreamState::EV].build_t0 : nullptr);
  e->word_off_cleared = true;
  e->build_stamped = h->prof;
  e->counts_preloaded = true; e->up_src_cnt.clear(); e->up_tgt_cnt.clear();
  // target build: against the stream's plan when there is one (no wait), else synchronously -- which makes the plan
  e->async_build = true;
  e->plan_cb = ss.plan_cb; e->plan_words = ss.plan_words;
  HIPCHK(h, e->d_words.reserve(e->plan_words));
  rc = mi355ndt_batch_build_targets(e);
  if (rc) { h->err = e->err; return rc; }
  if (!(e->plan_cb > 0 && e->plan_words > 0)) stream_learn_plan(ss, e);   // that build waited for its sizes
  if (ss.reserve_wg > 0) HIPCHK(h, hipEventRecord(ss.ev_built[ci], e->stream));
  stream_geometry(ss, e);
  gauss_constants3(h->prm.outlier_ratio, h->prm.resolution, h->gauss_last);
  S.busy = true;
  S.launch = ss.launches;
  rc = stream_launch(h, ci, n_pairs);
  if (rc) {                                          // the launch cannot be made (not resident): this and every later batch synchronously
    ss.sync_only = true;
    rc = stream_run_sync(h, S);
    if (rc) { S.busy = false; return rc; }
    S.done_sync = true;
  }
  e->aligned_once = true;
  *batch_id = id; ss.next_id++;
  return MI355NDT_OK;
}

// The stream for the caller the reference actually has: HOST clouds (scan_matching_odom_nodelet.cpp:144-183 receives pcl::PointCloud records, one
// callback at a time).  The batch's clouds are staged by the engine's own threads into the pinned slots of the context this batch lives in,
// cross PCIe on that context's copy streams and land in ITS device buffers -- while the launches of the batches submitted before keep the GPU
// busy -- and then the batch goes the way of mi355ndt_stream_submit.  Returns when the caller's memory is no longer needed.
int mi355ndt_stream_submit_host(mi355ndt_handle* h, int n_pairs, const void* const* targets, const size_t* target_counts, const void* const* sources,
                                const size_t* source_counts, size_t stride, const float* guesses, int n_threads, long long* batch_id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!h->ss) return MI355NDT_ERR_STATE;
  StreamState& ss = *h->ss;
  if (n_pairs < 1 || n_pairs > ss.max_pairs || !targets || !target_counts || !sources || !source_counts || stride < 12 || !guesses || !batch_id) return MI355NDT_ERR_BAD_ARG;
  for (int b = 0; b < n_pairs; b++)
    if (target_counts[b] > ss.max_tgt || source_counts[b] > ss.max_src || (!targets[b] && target_counts[b]) || (!sources[b] && source_counts[b])) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const int ci = (int)(ss.next_id % ss.nctx);
  StreamCtx& S = ss.ctx[ci];
  if (S.busy) { h->err = "stream_submit_host: collect batch " + std::to_string(S.batch_id) + " first (its context is the one this batch needs)"; return MI355NDT_ERR_STATE; }
  mi355ndt_handle* e = S.e.get();
  const size_t tp = (ss.max_tgt + 63) & ~(size_t)63, sp = (ss.max_src + 63) & ~(size_t)63;
  if (!e->d_tgt_own || !e->d_src_own || e->own_tgt_pairs < ss.max_pairs || e->own_src_pairs < ss.max_pairs || e->own_tgt_pitch != tp || e->own_src_pitch != sp) {
    int rc = mi355ndt_batch_reserve(e, ss.max_pairs, ss.max_tgt, ss.max_src);      // (once per context: the stream's sizes never change)
    if (rc) { h->err = e->err; return rc; }
  }
  // (the context's previous batch has been collected -- S.busy is false --, so no kernel still reads these rows)
  e->n_pairs = ss.max_pairs; e->d_tgt = e->d_tgt_own; e->d_src = e->d_src_own; e->tgt_pitch = tp; e->src_pitch = sp;
  int rc = mi355ndt_batch_set_clouds(e, 0, n_pairs, targets, target_counts, sources, source_counts, stride, n_threads);
  if (rc) { h->err = e->err; return rc; }
  std::vector<int> tc((size_t)n_pairs), sc((size_t)n_pairs);
  for (int b = 0; b < n_pairs; b++) { tc[(size_t)b] = (int)target_counts[b]; sc[(size_t)b] = (int)source_counts[b]; }
  // (the build that mi355ndt_stream_submit enqueues first waits for these uploads: uploads_before_compute of the context's engine)
  return mi355ndt_stream_submit(h, n_pairs, e->d_tgt_own, tc.data(), tp, e->d_src_own, sc.data(), sp, guesses, batch_id);
}

int mi355ndt_stream_pose_records(mi355ndt_handle* h, void* d_records, size_t capacity, int id_base, int id_stride) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!h->ss) return MI355NDT_ERR_STATE;
  if ((d_records && capacity == 0) || capacity > (size_t)MAX_PAIRS) return MI355NDT_ERR_BAD_ARG;
  StreamState& ss = *h->ss;
  ss.pose_next = d_records; ss.pose_cap_next = d_records ? capacity : 0; ss.pose_base_next = id_base; ss.pose_stride_next = id_stride;
  return MI355NDT_OK;
}

// a launch gave up (ctl->abort_): nothing it left behind can be trusted to continue from -- every unfinished batch is re-run synchronously
// by its collect, and the next launch starts without a hand-over list
static void stream_recover(mi355ndt_handle* h) {
  StreamState& ss = *h->ss;
  if (ss.build_stream) (void)hipStreamSynchronize(ss.build_stream);
  (void)hipStreamSynchronize(h->stream);
  CtxStat st[ASYNC_MAX_CTX];
  if (hipMemcpy(st, ss.d_stat, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) memset(st, 0, sizeof st);
  for (int c = 0; c < ss.nctx; c++) {
    StreamCtx& S = ss.ctx[c];
    if (S.busy && !S.done_sync && st[c].done != (unsigned)S.n_pairs) S.redo = true;
  }
  ss.drop_carry = true;
  ss.recovered_upto = ss.launches - 1;       // everything enqueued so far has drained and been marked: a later collect that reads this launch's abort flag again has nothing to do
  h->P.async_fallbacks++;
}

int mi355ndt_stream_collect(mi355ndt_handle* h, long long batch_id, mi355ndt_result* out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!h->ss) return MI355NDT_ERR_STATE;
  StreamState& ss = *h->ss;
  if (batch_id < 0 || batch_id >= ss.next_id || !out) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const int ci = (int)(batch_id % ss.nctx);
  StreamCtx& S = ss.ctx[ci];
  if (!S.busy || S.batch_id != batch_id) return MI355NDT_ERR_BAD_ARG;       // collected already (or its context has been recycled)
  mi355ndt_handle* e = S.e.get();
  bool reran = S.done_sync;                          // went through the synchronous path (then the pose records come from the engine's packer)
  if (!S.done_sync) {
    long long j = S.launch;
    bool plan_exceeded = false;
    for (;;) {
      int rc = stream_wait_launch(h, j);
      if (rc) return rc;
      const StreamStatus st = *const_cast<const StreamStatus*>(ss.h_status + (j % StreamState::EV));
      if (st.abort_ && !S.redo && j > ss.recovered_upto) stream_recover(h);
      plan_exceeded = st.ctx[ci].plan_exceeded != 0;
      if (S.redo || plan_exceeded) break;
      if (st.ctx[ci].done == (unsigned)S.n_pairs) break;
      if (j + 1 < ss.launches) { j++; continue; }  // its stragglers ride in a later launch that is already queued
      rc = stream_launch(h, -1, 0);                  // nothing newer: flush them
      if (rc) { stream_recover(h); S.redo = true; break; }
      j = ss.launches - 1;
    }
    if (S.redo || plan_exceeded) {
      // the batch did not fit the build plan (its grids were withheld), or its launch gave up: the synchronous path, which also re-makes the plan
      const int rc = stream_run_sync(h, S);
      if (rc) { S.busy = false; return rc; }
      h->P.stream_redone++;
      reran = true;
    }
  }
  if (S.d_pose && reran) {       // a batch that went through the synchronous path: its records from the engine's packer
    int rc = mi355ndt_batch_pose_records(e, S.pose_base, S.pose_stride, S.d_pose, (size_t)S.pose_cap);
    if (rc) { h->err = e->err; return rc; }
  }
  memcpy(out, S.h_res, (size_t)S.n_pairs * sizeof(mi355ndt_result));
  tolerance_warnings(h, out, S.n_pairs);         // (a synchronously re-run batch has them already: idempotent)
  account_sweeps(h, out, e->h_src_cnt.data(), S.n_pairs, neighbor_K(h->prm.neighbor_mode));
  S.busy = false;
  return MI355NDT_OK;
}

int mi355ndt_pack_pose_records(const mi355ndt_result* results, int n, int id_base, int id_stride, void* records, size_t capacity) {
  if (!results || !records || n < 0 || (size_t)n > capacity) return MI355NDT_ERR_BAD_ARG;
  PoseRecord* out = (PoseRecord*)records;
  for (size_t k = 0; k < capacity; k++) {
    PoseRecord r;
    memset(&r, 0, sizeof r);
    r.pair_id = -1;
    if (k < (size_t)n) {
      for (int a = 0; a < 16; a++) r.final_cm[a] = results[k].final_colmajor[a];
      r.score = (float)results[k].score;
      r.iterations = results[k].iterations;
      r.converged = results[k].converged;
      r.pair_id = id_base + (int)k * id_stride;
    }
    out[k] = r;
  }
  return MI355NDT_OK;
}
