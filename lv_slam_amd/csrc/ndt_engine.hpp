// ndt_engine.hpp -- the engine behind a handle: StreamCtx / StreamState / mi355ndt_handle, the error and state macros, the constants, and the
// one home of every decision about a configuration that more than one surface takes (neighbor_K, async_served, launch_slots, ...) and of the
// two writers of the slots' cloud bookkeeping (cloud_changed, clouds_reset).
#pragma once

// ------------------------------------------------------------------------------------ host side
// Ownership: every buffer, pinned block, stream and event the engine allocates lives in an owner of ndt_hostmem.hpp and is released with it.
// Raw pointers below are views into memory some owner (or the caller) holds; their comments say which.
struct mi355ndt_handle;
struct EngineDel { void operator()(mi355ndt_handle* e) const { (void)mi355ndt_destroy(e); } };

// ---- stream mode (mi355ndt_stream_*, the parent handle): n_contexts batches resident, one persistent launch per submitted batch,
// the stragglers of a launch carried into the next one (ndt_async.hpp).  One StreamState per session: mi355ndt_stream_begin creates it,
// mi355ndt_stream_end releases it.
struct StreamCtx {
  long long batch_id = -1; int n_pairs = 0;
  bool busy = false;                            // submitted, not yet collected
  bool redo = false;                            // collect re-runs it synchronously (its launch gave up)
  bool done_sync = false;                       // processed synchronously inside submit (configuration the one-launch align does not serve)
  long long launch = -1;                        // the launch that started it
  // a batch's small inputs -- target counts, source counts, guesses -- travel as ONE copy: pinned staging block -> device block, into which
  // the context engine's d_tgt_cnt / d_src_cnt / d_guess point
  DevBuf<int> d_in; PinBuf<int> h_in; unsigned* h_in_dev = nullptr;   // (h_in is mapped: the device reads it itself; h_in_dev views it)
  // results: MAPPED host memory -- a pair's result record is written there by the updater that finalises it (posted PCIe writes), no copy
  PinBuf<mi355ndt_result> h_res; mi355ndt_result* d_res_map = nullptr;   // (d_res_map: the device's view of h_res)
  std::vector<float> guesses;                   // (kept for a synchronous re-run)
  PoseRecord* d_pose = nullptr; int pose_cap = 0, pose_base = 0, pose_stride = 1;   // mi355ndt_stream_pose_records (this batch's gather block)
  std::unique_ptr<mi355ndt_handle, EngineDel> e;   // the context's own engine: bound clouds, grids, pair states (runs on the parent's stream)
};
struct StreamState {
  static constexpr int EV = 16;
  bool sync_only = false, drop_carry = true;
  int nctx = 0, max_pairs = 0, items = 0, ring_cap = 0, thresh = 0;
  bool thresh_given = false;                    // MI355NDT_OPT_STREAM_THRESHOLD or MI355NDT_STREAM_THRESH named the threshold (else automatic: capped per batch, stream_launch)
  size_t max_tgt = 0, max_src = 0;              // what mi355ndt_stream_begin was told (mi355ndt_stream_submit_host sizes the contexts' own cloud buffers with it)
  int plan_cb = 0; size_t plan_words = 0;
  void* pose_next = nullptr; size_t pose_cap_next = 0; int pose_base_next = 0, pose_stride_next = 1;   // apply to the next submit of this session
  long long next_id = 0, launches = 0, counted = 0;
  long long recovered_upto = -1;                // launches up to this one have had their abort handled (stream_recover runs once per aborted launch, not once per collect that walks past its slot)
  DevBuf<AsyncCtl> d_ctl;                       // two control blocks: a launch reads the hand-over list of the previous one
  DevBuf<int> d_ring;
  DevBuf<CtxStat> d_stat;                       // per context: pairs finalised, sizes and verdict of its last planned build
  // Build under the launch: with reserve_wg > 0 the contexts' engines run their builds on build_stream, the persistent launches leave
  // that many workgroup slots free, and events order  launch j-2 done -> build of batch j -> launch j
  HipStream build_stream; int reserve_wg = 0, launch_slots = 0;
  bool lean = false;                            // the last launch ran the lean item body (three waves per SIMD; decided per launch: stream_launch)
  bool reserve_given = false;                   // MI355NDT_OPT_STREAM_RESERVE or MI355NDT_STREAM_RESERVE named the reserve (else the defaults, per geometry)
  int last_reserve = 0, last_slots = 0;         // reserved slots and workgroups of the last launch that started a batch (before the first: the session's sizing)
  HipEvent ev_built[ASYNC_MAX_CTX], ev_launched[EV], ev_prepared[EV]; bool prep_first = true;
  PinBuf<volatile StreamStatus> h_status; StreamStatus* d_status = nullptr;   // mapped ring of per-launch status slots (k_stream_status); d_status: the device's view
  StreamCtx ctx[ASYNC_MAX_CTX];                 // (last: the contexts' engines are released before the stream they run on)
};

// ---- scratch of the sort-and-compact chain: stage clouds -> extremes -> grid -> keys -> one-segment radix sort -> run heads -> exclusive
// scan -> emit -> count.  The prefilter, the batch prefilter (K clouds at once, a segment each), the outlier removal (the batch form: K staged clouds in `x`, their index pools in `out`), the map cloud (both routes), the window map and the cloud index builds
// (kfi_build_rows: the keyframe fitness scores, GICP) share this one instance; results (d_pf_out, the keyframe store, the indexes) are not in it.
// Sharing is safe because
//   * every user enqueues its kernels, table copies and read-backs on h->stream, so stream order separates one user's work from the next's;
//   * every user waits for the stream before it returns, except mi355ndt_window_keyframe, whose trailing k_kf_emit still reads x, keys, vals,
//     flag and pos: only kernels on h->stream write those, so stream order covers it as well;
//   * `in` alone is written from the copy streams: its readers (k_pfb_*, k_pfa_*, k_mc_transform, k_kf_window) have finished when their call returns,
//     and uploads_before_compute / compute_enqueued order the uploads against the compute stream as they do for the batch rows;
//   * the pinned blocks are written by the host only at the start of a call, after vs_reserve has waited out a copy that may still read
//     them (`pending`), and read by the host only after the call's own wait.
// Growth: vs_reserve (ndt_host_voxel.hpp), the one place that re-allocates a member.
struct VoxelScratch {
  DevBuf<float> in, x, out;                       // staged SoA rows (upload_items) / moved points / the map cloud's centres
  DevBuf<unsigned char> keep;                     // per point: kept (the map cloud: finite)
  DevBuf<unsigned> keys, vals;                    // two of each per point (sort ping-pong); the map cloud: low / high words of its codes
  DevBuf<unsigned> hist, offs, tmp;               // radix sort tile histograms / offsets, scan chunk totals
  DevBuf<int> flag, pos;                          // run heads, their exclusive scan.  pos grows last: its capacity vouches for every per-point member
  DevBuf<int> mm, cnt, aabb, stat;                // six extreme words (k_minmax / k_kfi_begin take them as unsigned), a point count, the map
                                                  // cloud's per-chunk boxes, the index builds' status and count words
  DevBuf<PfGrid> grid; DevBuf<McBox> box;
  DevBuf<unsigned char> tab; PinBuf<unsigned char> h_tab;   // per-call tables (scan / keyframe table + poses; edges + item tables) and their pinned twin
  DevBuf<double> part; PinBuf<double> h_part;     // block partials of the keyframe fitness kernels
  PinBuf<int> h_ret;                              // pinned landing words (counts, statuses)
  bool pending = false;                           // a copy out of h_tab is enqueued and the stream has not been waited for since
};

// ---- the spatial index of one resident cloud (ndt_kffitness.hpp: lattice, occupancy words, run starts, the points and their ids in cell
// order -- one block), built by kfi_build_rows (ndt_host_kffitness.hpp) for whichever surface searches the cloud first.  status: NO_INDEX,
// else the lattice's GRID_* status; n_fin: the cloud's searchable points -- both as the host learned them at the end of the call that built it.
struct CloudIndex {
  static constexpr int NO_INDEX = -1;
  DevBuf<unsigned char> blob; int status = NO_INDEX; int n_fin = 0;
};

// ---- GICP (mi355ndt_gicp_*, ndt_gicp.hpp / ndt_host_gicp.hpp): what the surface keeps per cloud beside its index -- the nine f64 covariance
// rows, keyed by the (k_correspondences, gicp_epsilon) they were computed with.  A host cloud's live with the surface's side, a keyframe's
// with the keyframe (released with it).
struct GicpCache {
  DevBuf<double> cov;
  int k = -1; double eps = 0.0;                   // what cov holds (k < 0: nothing)
};
struct GicpSide {
  DevBuf<float> rows_own; size_t n = 0, pitch = 0; // a host cloud's rows ([3][pitch], the tail zeroed)
  int kf_id = -1; bool set = false;               // kf_id >= 0: the rows, the index and the cache are the keyframe's
  CloudIndex index; GicpCache cache;              // a host cloud's
};

struct mi355ndt_handle {
  int device = 0;
  HipStream own_stream;                         // the engine's compute stream, unless mi355ndt_set_stream gave it one
  hipStream_t stream = nullptr;                 // view: own_stream or the caller's stream
  mi355ndt_params prm;
  std::string err;

  int n_pairs = 0, cap_pairs = 0;
  size_t tgt_pitch = 0, src_pitch = 0;          // geometry in use
  size_t own_tgt_pitch = 0, own_src_pitch = 0;  // geometry of the owned buffers
  int own_tgt_pairs = 0, own_src_pairs = 0;
  DevBuf<float> d_tgt_own, d_src_own;
  const float *d_tgt = nullptr, *d_src = nullptr;   // views: d_tgt_own / d_src_own or a device buffer bound by the caller
  DevBuf<int> d_tgt_cnt_own, d_src_cnt_own;
  int *d_tgt_cnt = nullptr, *d_src_cnt = nullptr;   // views: d_tgt_cnt_own / d_src_cnt_own or the stream context's input block
  std::vector<int> h_tgt_cnt, h_src_cnt;
  std::vector<int> up_tgt_cnt, up_src_cnt;        // what d_tgt_cnt / d_src_cnt currently hold (uploads are skipped when unchanged)
  // the slots' intensity, a plane per side beside the rows: [slot][pitch], made by the first mi355ndt_batch_prefilter with an intensity that
  // touches the side, dropped by mi355ndt_batch_reserve; and per slot whether its row holds the cloud's intensity -- set by that prefilter, kept
  // by mi355ndt_batch_remove_outliers, cleared by every other route that fills the slot (cloud_changed / clouds_reset, below)
  DevBuf<float> d_tgt_i, d_src_i;
  std::vector<unsigned char> tgt_has_i, src_has_i;
  bool have_target = false, have_source = false;  // written by cloud_changed / clouds_reset (below) alone, with the host counts
  GridsBuilt built{};                             // what the resident grids hold (ndt_grid_state.hpp): filled at the end of build_targets_impl, asked by ensure_grids
  bool aligned_once = false;                      // d_state / d_results hold the outcome of an align of the CURRENT batch

  // build workspace
  unsigned* d_minmax = nullptr;                  // view: a slice of d_word_off (zeroed together before every build)
  DevBuf<GridDesc> d_grid;
  DevBuf<unsigned> d_nwords, d_word_off;
  DevBuf<unsigned> d_keys_a, d_keys_b;           // cell key per target point: unsorted / sorted (segment-local radix sort)
  DevBuf<unsigned> d_vals_a, d_vals_b;
  DevBuf<BitWord> d_words;
  size_t recs_per_pair = 0;                      // voxel records per target of the records group (d_recs ... d_cent); 0: group not allocated
  DevBuf<VoxelRec> d_recs; DevBuf<int> d_vox_idx, d_vox_n;
  DevBuf<unsigned> d_seg_start; DevBuf<double> d_sums;
  DevBuf<unsigned> d_heads, d_head_cnt;          // k_mark's run heads per slice
  DevBuf<float> d_cent; DevBuf<double> d_icov64;
  DevBuf<int> d_kdw;                             // per-leaf weights for ndt_pca + KDTREE (dead leaves included)
  DevBuf<float4> d_sorted; bool leaf_sorted = false;   // MI355NDT_LEAF_SORTED: the sorted order as points (k_sorted_points)
  DevBuf<unsigned> d_rs_hist, d_rs_offs;         // segmented radix sort: tile histograms / offsets
  // fitness scores (one pair or a batch, fit_scores): the block partials; the occupied-cell index of every target (ndt_fitness.hpp), built on the
  // first call after a target build; the launch's item table and transforms
  DevBuf<double> d_fit;
  DevBuf<BitWord> d_fwords; DevBuf<unsigned> d_fruns;
  DevBuf<int> d_fit_items; DevBuf<float> d_fit_T;
  // prefilter result (mi355ndt_use_prefiltered reads it after any number of other calls): [pf_ch][pf_pitch], x, y, z and -- pf_ch == 4, a
  // prefilter called with an intensity offset -- the intensity
  DevBuf<float> d_pf_out; int pf_count = 0; size_t pf_pitch = 0; int pf_ch = 3;
  int pf_ioff = -1;                               // ... at this byte offset of the input's records, where the read-backs write it
  bool pf_resident = false;                       // a prefilter call has left a result (an empty one owns no rows)
  // outlier removal over it (mi355ndt_prefilter_outliers): the index rebuilt by every call, dist[] and its pinned twin
  CloudIndex ol_index; DevBuf<float> d_ol_dist; PinBuf<float> h_ol_dist;
  int ol_cell_mm = 100;                           // MI355NDT_OPT_OUTLIER_CELL_MM
  int pf_group = 0;                               // MI355NDT_OPT_PREFILTER_GROUP: raw clouds per group of mi355ndt_batch_prefilter (0: by the scratch budget)
  VoxelScratch vs;                                // scratch of the prefilter, the map cloud, the window map and the keyframe index builds
  // keyframe store (mi355ndt_keyframe_*, mi355ndt_window_keyframe): every keyframe owns its rows -- [3 or 4][pitch] floats, x, y, z and, when
  // carried, the intensity; pitch = count rounded up to 64, the tail zeroed -- under an id that is never given out twice
  // ... and, once it has been the searched side of mi355ndt_keyframe_fitness_scores or a cloud of the GICP surface, its one spatial index,
  // kept until the keyframe is released.
  struct Keyframe {
    DevBuf<float> rows; size_t n = 0, pitch = 0; int ch = 3;
    CloudIndex index;
    GicpCache gicp;                               // the GICP surface's covariances over this keyframe, once it has been one of its clouds
  };
  std::map<int, Keyframe> keyframes;
  int kf_next_id = 0;
  int kff_cell_mm = 100;                          // MI355NDT_OPT_KF_FITNESS_CELL_MM
  // GICP surface: parameters, the two clouds, the resident correspondences (idx, M SoA over the source's pitch), the sweep's chunk partials,
  // the mapped result record the host reads after every evaluation, the last final transformation
  struct Gicp {
    mi355ndt_gicp_params prm{20, 1e-3, 2e-3, 5e-4, 200, 20, 5.0};
    GicpSide side[2];
    DevBuf<int> idx, m; DevBuf<double> maha, part; DevBuf<float> moved;
    PinBuf<double> h_rec; double* d_rec = nullptr;   // (h_rec is mapped; d_rec: the device's view)
    bool have_corr = false, have_final = false; int n_matched = 0;
    float final_cm[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
  } gicp;
  // GICP batch (mi355ndt_gicp_batch_*, ndt_host_gicp_batch.hpp): the candidates of one loop check against the surface's target.  A slot is a
  // source side (a host cloud's rows, index and cache, or a keyframe id) with correspondences, chunk partials and a final transformation of
  // its own; the slots share one block of match counters, one mapped block of result records and the round's table (pinned twin -> device).
  struct GicpBatch {
    struct Slot {
      GicpSide side;
      DevBuf<int> idx; DevBuf<double> maha, part;
      bool have_final = false; float final_cm[16];
    };
    std::vector<Slot> slot;
    DevBuf<int> m;
    PinBuf<double> h_rec; double* d_rec = nullptr;   // (h_rec is mapped; d_rec: the device's view)
    PinBuf<GcSlot> h_tab; DevBuf<GcSlot> d_tab;
    int rounds = 0; std::vector<int> requests;      // of the last batch align
  } gicp_batch;
  // ICP surface (mi355ndt_icp_*, ndt_host_icp.hpp): parameters, the two clouds (a target's index is its side's or its keyframe's; a source
  // needs none), the working cloud W ([3][pitch], the surface's own: a keyframe source is never written) with its correspondences, the
  // step's chunk partials and match counter, the mapped record the host reads after every step, the last run (its final transformation
  // and the estimate W has not been moved by yet)
  struct IcpWork {
    DevBuf<float> W, d2; DevBuf<int> idx; DevBuf<double> part;
    size_t n = 0, pitch = 0;                        // of the cloud W holds
    bool have_final = false; IcpRun run;
  };
  struct Icp {
    mi355ndt_icp_params prm{0.0, 10, -DBL_MAX, 1.3407807929942596e154, 3, 0};
    GicpSide side[2];
    IcpWork work;
    DevBuf<int> m; DevBuf<float> moved;
    PinBuf<double> h_rec; double* d_rec = nullptr;   // (h_rec is mapped; d_rec: the device's view)
  } icp;
  // ICP batch (mi355ndt_icp_batch_*, ndt_host_icp_batch.hpp): the candidates of one loop check against the surface's target.  A slot is a
  // source side with a working cloud of its own; the slots share one block of match counters, one mapped block of records and the round's
  // table (pinned twin -> device).
  struct IcpBatch {
    struct Slot { GicpSide side; IcpWork work; };
    std::vector<Slot> slot;
    DevBuf<int> m;
    PinBuf<double> h_rec; double* d_rec = nullptr;
    PinBuf<IcpSlot> h_tab; DevBuf<IcpSlot> d_tab;
    int rounds = 0; std::vector<int> requests;      // of the last batch align
  } icp_batch;
  float last_final[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
  PinBuf<unsigned> h_pin_u;                      // pinned scratch (2 unsigned)

  // align workspace
  DevBuf<PairState> d_state;
  DevBuf<double> d_partials;
  int chunks_per_pair = 0;
  int rows_per_pair = 0, pts_per_chunk = CHUNK_PTS;   // stored partial rows per pair / points covered by one chunk of k_update's tree
  int items_per_pair = 0;                         // sweep work items per pair (= rows_per_pair in batch mode, 4 x rows_per_pair in latency mode)
  bool async_force = false;                       // MI355NDT_OPT_ASYNC_ALIGN = 2 / MI355NDT_ASYNC=2: the one-launch align also for batches smaller than the resident waves (tests, fuzzing)
  bool async_align = true;                        // MI355NDT_OPT_ASYNC_ALIGN: batch aligns as ONE persistent launch (ndt_async.hpp); MI355NDT_ASYNC=0 turns it off
  int score_only_last = 1;                        // MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP: the one-launch align's last sweep of a pair evaluates the score alone
  DevBuf<int> d_ring; DevBuf<unsigned> d_arrived; DevBuf<AsyncCtl> d_actl;
  PinBuf<AsyncCtl> h_pin_actl;
  DevBuf<AsyncTab> d_atab;                        // the launch's context table (ndt_async.hpp)
  unsigned debug_abort_pos = 0xFFFFFFFFu;         // MI355NDT_OPT_DEBUG_ASYNC_ABORT (test hook): the wave that claims this position of ring 0 gives up
  unsigned debug_ring_mask = 0xFFu;               // MI355NDT_OPT_DEBUG_ASYNC_RINGS (test hook): rings whose workgroups take part
  int sweep_waves = 0;                            // MI355NDT_OPT_SWEEP_WAVES: 0 = automatic (async_lean, ndt_host_sweep.hpp), 2, 3
  int last_async_wpe = 0, last_async_grid = 0;    // the last persistent launch: its kernel's waves per SIMD, its workgroups (mi355ndt_profile)
  int arith = 0;                                  // MI355NDT_OPT_ARITH: 0 = the reference recipe's arithmetic, one rounding per operation; 1 = tolerance arithmetic (ndt_sweep.hpp: eval_hit_fast)
  DevBuf<VoxelRecF> d_recs_fast;                  // ... and the records its sweeps read (k_voxels writes them beside d_recs)
  int pose_model = 0;                             // MI355NDT_OPT_POSE_MODEL: 0 = ndt_omp_impl2.hpp (SE(3) tangent), 1 = ndt_omp_impl.hpp (Euler angles; ndt_grid_state.hpp says what it serves)
  int ground_class = 0;                           // MI355NDT_OPT_GROUND_CLASS: 0 = off; 1 / 2 / 3 = pclomp_ground's flag_class 1 / 2 / 0 (ndt_grid_state.hpp says what it serves)
  DevBuf<unsigned char> d_leaf_class;             // ... and, for 1 / 2, the class code of every leaf record (k_voxels writes it beside d_recs; SweepConst::leaf_class)
  int ndt_class = 0;                              // MI355NDT_OPT_NDT_CLASS: 0 = pclomp's class (pose_model says which implementation), 1 = pcl::NormalDistributionsTransform (f64; ndt_grid_state.hpp)
  DevBuf<double> d_pcl_rows;                      // ... and its per-pair rows as doubles, EULER_ROW_WORDS a pair slot (SweepConst::pcl_rows)
  DevBuf<float> d_euler_rows;                     // ... and its per-pair rows, EULER_ROW_WORDS floats a pair slot (SweepConst::euler_rows)
  int f32_sum_order = 0;                          // MI355NDT_OPT_F32_SUM_ORDER: 0 = (t0 + t1) + t2 (canonical), 1 = (t0 + t2) + t1 (Eigen 3.3 SSE predux pairing)
  double gauss_last[3] = {0, 0, 0};               // gauss_d1_/d2_/d3_ as the constructor / the last computeTransformation left them (calculateScore reads them)
  DevBuf<float> d_score_pts; DevBuf<double> d_score_part;   // calculateScore workspace
  bool latency_mode = false;                      // mi355ndt_set_latency_mode
  bool seq_running = false;                       // inside mi355ndt_sequence_run
  int fine_it = 0;                                // 0: batch-mode sweep items (512 points); 1 / 2: fine items of fine_it * 64 points (latency mode)
  int fine_tiles = 2;                             // MI355NDT_FINE_TILES overrides (tuning runs)
  int dyn_shift = -1;                             // < 0: per search mode (make_sweep_const); MI355NDT_SWEEP_DYN_SHIFT overrides (tuning runs)
  DevBuf<int> d_grid_of;                          // sequence mode: grid index per pair
  const int* d_grid_of_use = nullptr;             // what the sweeps are given: view of d_grid_of inside mi355ndt_sequence_run, else null (pair b -> grid b)
  DevBuf<SeqState> d_seq; DevBuf<mi355ndt_seq_frame> d_seq_out; DevBuf<double> d_stamps;
  PinBuf<volatile int> h_seq_flags; int* d_seq_flags = nullptr;   // mapped pinned: [0] = run finished, [1] = update launches executed; d_seq_flags: the device's view
  DevBuf<float> d_guess_own;
  float* d_guess = nullptr;                       // view: d_guess_own or the stream context's input block
  PinBuf<float> h_pin_guess;                      // pinned staging copy of the caller's guesses (no sync needed after the upload)
  DevBuf<mi355ndt_result> d_results;
  DevBuf<int> d_active;                           // per-round active counters
  DevBuf<int> d_active_list;                      // pairs taking part in the next sweep (compacted by k_update)
  DevBuf<SweepCtl> d_ctl;                         // two control blocks: the sweep reading one zeroes the other for the next round
  int ctl_idx = 0;                                // block the NEXT sweep reads (k_init_state / k_update fill it)
  int n_cu = 256;
  PinBuf<int> h_pin_active;
  HipEvent ev_burst[2];                           // one per in-flight burst of align rounds
  DevBuf<unsigned long long> d_hits;              // [0] (point,voxel) evaluations, all sweeps; [1] score-only sweeps of the one-launch align
  // mi355ndt_batch_score_poses (ndt_host_pose_scores.hpp): the call's tables (pinned twin -> device), its rows and its mapped landing block
  // (n scores, n hit counts) -- all its own: the align workspace above is not touched
  struct PoseScores { PinBuf<unsigned char> h_tab; DevBuf<unsigned char> d_tab; DevBuf<double> d_rows; PinBuf<double> h_out; } pose_scores;
  DevBuf<float> d_hook;                           // 16 + 9 floats, 6 doubles
  DevBuf<float> d_aligned;
  PinBuf<float> h_pin_aligned;                    // pinned landing buffer of get_aligned
  // host-cloud uploads: a ring of pinned staging slots, a copy stream of its own, a device staging buffer per slot.  The caller's
  // records are compacted to x,y,z into a slot (the only CPU work), the slot goes over PCIe asynchronously and a small kernel
  // spreads it into the SoA rows; the next call stages the next cloud while this one is still in flight.
  struct UpSlot { PinBuf<float> h; DevBuf<float> d; HipEvent ev; bool used = false, filling = false; };   // h, d: 3 floats per point
  static constexpr int UP_SLOTS = 12;             // (a slot grows to the largest transfer it has carried: up to UP_GROUP_MAX clouds = 12.6 MB of 65,536-point clouds)
  UpSlot up[UP_SLOTS];
  int up_next = 0;
  static constexpr int UP_STREAMS = 4;            // an upload rides copy stream (pair + 2 * side) % UP_STREAMS: per-transfer latencies of the SDMA queues
                                                  // overlap across pairs, uploads into the same rows stay ordered
  HipStream copy_stream[UP_STREAMS];
  HipEvent ev_uploads[UP_STREAMS], ev_compute;    // copy streams -> compute stream, compute stream -> copy streams
  bool uploads_pending = false;
  std::mutex up_mtx;                              // batch_set_target / batch_set_source may be called from several threads (distinct pairs)

  // asynchronous target build (stream mode: the engine is one batch context of a parent handle).  A build normally waits for two words
  // from the device -- the bitmap words of all grids (pool size) and the largest grid (sort key width); with a PLAN from earlier builds of
  // the stream it does not: it sorts plan_cb key bits, clears plan_words pool words, and k_build_check turns every grid of the batch into
  // "no grid" (and raises its flag in d_bstat) should the batch not fit the plan -- the parent then re-runs that batch synchronously and learns.
  bool async_build = false;
  int plan_cb = 0; size_t plan_words = 0;
  unsigned* d_bstat = nullptr;                    // view: the parent's CtxStat of this context -- [1] total words, [2] largest grid, [3] plan exceeded
  bool counts_preloaded = false;                  // the parent has put this batch's point counts (and guesses) on the device already
  bool build_stamped = false;                    // stream mode + profiling: build times come from stamps in the launch's status slot, not from events
  bool word_off_cleared = false;                 // stream mode: k_stream_inputs has cleared d_word_off for the next build (no fill)

  // stream mode: the session (null outside mi355ndt_stream_begin ... mi355ndt_stream_end) and the options it starts with
  std::unique_ptr<StreamState> ss;
  int s_thresh_opt = -1;                          // MI355NDT_OPT_STREAM_THRESHOLD
  int s_reserve_opt = -1;                         // MI355NDT_OPT_STREAM_RESERVE

  // profiling
  bool prof = false;
  mi355ndt_profile P{};
  struct EvSpan { hipEvent_t first, second; bool first_shared; };   // first_shared: `first` is the previous span's `second`
  std::vector<EvSpan> ev_sweep, ev_update, ev_build;
  hipEvent_t ev_last = nullptr;                   // end event of the span just closed, reusable as the next span's begin while
  bool ev_last_fresh = false;                     // nothing else has been enqueued on the stream since
  std::vector<hipEvent_t> ev_pool;                // idle timing events (filled by mi355ndt_profile_enable)
  size_t ev_pool_target = 4096;

  ~mi355ndt_handle() {                            // (the profiling pool is not held by owners: its events move between the pool and the spans)
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    for (auto* v : {&ev_sweep, &ev_update, &ev_build})
      for (auto& e : *v) { if (!e.first_shared) (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  }
};

#define HIPCHK(h, call)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                              \
      return MI355NDT_ERR_HIP;                                                                   \
    }                                                                                            \
  } while (0)

// several kernels carry the pair index in grid.y (HIP limit 65535)
#define MAX_PAIRS 65535
#ifndef UP_GROUP_PAIRS
#define UP_GROUP_PAIRS 8          // pair slots per upload group of mi355ndt_batch_set_clouds: their targets and sources travel as ONE transfer (measured, 271-pair
#endif                            // batches of 32-byte records streamed: 2 / 4 / 8 pairs per transfer = 20.2 / 21.4 / 22.2 k registrations/s; one cloud per transfer: 15.4 k)
#define UP_GROUP_MAX   (2 * UP_GROUP_PAIRS)
static_assert(UP_GROUP_MAX <= (int)(sizeof(DeintTab::e) / sizeof(DeintTab::e[0])), "k_deinterleave_multi's table");
// between mi355ndt_stream_begin and mi355ndt_stream_end the handle's batches belong to the stream: the other entry points refuse
#define NOT_IN_STREAM(h) do { if ((h)->ss) { (h)->err = "the handle is in stream mode (mi355ndt_stream_begin): call mi355ndt_stream_end first"; return MI355NDT_ERR_STATE; } } while (0)
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield");
#endif
}
static int ceil_log2(unsigned v) { int b = 0; while ((1u << b) < v) b++; return b; }

// neighbour search mode -> cells probed per point (KDTREE: the 27-cell block + centroid radius test)
static int neighbor_K(int mode) { return mode == MI355NDT_DIRECT1 ? 1 : mode == MI355NDT_DIRECT7 ? 7 : mode == MI355NDT_DIRECT26 ? 26 : 27; }
static void build_offsets(int mode, SweepConst& sc) {
  sc.K = neighbor_K(mode);
  sc.table = sc.K == 1 ? 0 : sc.K == 7 ? 1 : 2;
}

static void gauss_constants3(double outlier_ratio, float resolution, double d[3]) {
  // ndt_omp_impl2.hpp:93-100 (and the constructor, impl2:70-76)
  double c1 = 10 * (1 - outlier_ratio);
  double c2 = outlier_ratio / pow((double)resolution, 3);
  d[2] = -log(c2);
  d[0] = -log(c1 + c2) - d[2];
  d[1] = -2 * log((-log(c1 * exp(-0.5) + c2) - d[2]) / d[0]);
}
static void gauss_constants(const mi355ndt_params& p, double& d1, double& d2) {
  double d[3];
  gauss_constants3(p.outlier_ratio, p.resolution, d);
  d1 = d[0]; d2 = d[1];
}

static int check_params(const mi355ndt_params& p) {
  if (!(p.resolution > 0) || !std::isfinite(p.resolution)) return MI355NDT_ERR_BAD_ARG;
  if (p.neighbor_mode < 0 || p.neighbor_mode > 3) return MI355NDT_ERR_BAD_ARG;
  if (p.variant < 0 || p.variant > 1) return MI355NDT_ERR_BAD_ARG;
  if (p.min_points_per_voxel < 1) return MI355NDT_ERR_BAD_ARG;
  if (p.max_iterations < 0) return MI355NDT_ERR_BAD_ARG;
  return MI355NDT_OK;
}

// does the tolerance arithmetic (MI355NDT_OPT_ARITH = 1) serve this engine's configuration?  (mt_is_live, is_pca_kd, grid_extras: ndt_grid_state.hpp)
// the pose model, the arithmetic and the grid extras of this engine's aligns, class and options taken together (ndt_grid_state.hpp)
static int eff_model(const mi355ndt_handle* h) { return class_model(h->ndt_class, h->pose_model); }
static int eff_ground(const mi355ndt_handle* h) { return h->ground_class; }
static GridExtras eff_extras(const mi355ndt_handle* h, bool live = false) {
  return grid_extras(h->prm, model_arith(h->pose_model, h->arith, h->ndt_class, h->ground_class), live, h->ndt_class, h->ground_class);
}
static bool fast_served(const mi355ndt_handle* h) { return eff_extras(h).recs_fast; }
// the rows of the Euler model for this align's pairs, or null under model 0: what the set-up kernels, k_update and the sweeps are given
static float* euler_rows_of(const mi355ndt_handle* h) { return eff_model(h) == POSE_MODEL_EULER ? h->d_euler_rows.p : nullptr; }
// ... and the rows as doubles under MI355NDT_OPT_NDT_CLASS = 1 (then the writers fill these and leave the f32 ones alone), else null
static double* pcl_rows_of(const mi355ndt_handle* h) { return h->ndt_class == NDT_CLASS_PCL ? h->d_pcl_rows.p : nullptr; }
// a surface model 1 does not serve at all (sequence runs, streams, computeHessian, an explicit sweep pose)
#define NOT_EULER(h, what) do { \
    if ((h)->ndt_class == NDT_CLASS_PCL) { (h)->err = what ": not served under MI355NDT_OPT_NDT_CLASS = 1"; return MI355NDT_ERR_UNSUPPORTED; } \
    if ((h)->pose_model == POSE_MODEL_EULER) { (h)->err = what ": not served under MI355NDT_OPT_POSE_MODEL = 1"; return MI355NDT_ERR_UNSUPPORTED; } \
    if ((h)->ground_class != GROUND_CLASS_NONE) { (h)->err = what ": not served under a non-zero MI355NDT_OPT_GROUND_CLASS"; return MI355NDT_ERR_UNSUPPORTED; } } while (0)

// "Do the grids serve this call?" -- asked by ensure_grids (ndt_host_build.hpp) and nowhere else; it builds the wanted flavour when they do not.
//   GRIDS_ANY     any valid grid will do (the fitness scores read the base records alone); none: this configuration's is built
//   GRIDS_CONFIG  what this configuration's sweeps read (the aligns, the derivative hooks, mi355ndt_set_params)
//   GRIDS_LIVE    the flavour of a live More-Thuente loop, f32 centroids + f64 inverse covariances (calculateScore, computeHessian)
enum GridWant { GRIDS_ANY, GRIDS_CONFIG, GRIDS_LIVE };
static int ensure_grids(mi355ndt_handle* h, GridWant want);
// A slot's cloud changed: `n` consecutive slots of one side from `first_pair` now hold counts[0 .. n) points.  A new target leaves the grids
// describing a cloud that is gone.  (Under up_mtx: mi355ndt_batch_set_target / _source may run on several threads, distinct pairs.)
// has_intensity: the slots' intensity rows hold these clouds' intensities (the batch prefilter, the outlier removal over such a slot).
template <typename N>
static void cloud_changed(mi355ndt_handle* h, bool tgt, int first_pair, int n, const N* counts, bool has_intensity = false) {
  std::lock_guard<std::mutex> lk(h->up_mtx);
  std::vector<int>& cnt = tgt ? h->h_tgt_cnt : h->h_src_cnt;
  std::vector<unsigned char>& has_i = tgt ? h->tgt_has_i : h->src_has_i;
  has_i.resize(cnt.size(), 0);
  for (int k = 0; k < n; k++) { cnt[(size_t)(first_pair + k)] = (int)counts[k]; has_i[(size_t)(first_pair + k)] = has_intensity ? 1 : 0; }
  (tgt ? h->have_target : h->have_source) = true;
  if (tgt) h->built.valid = false;
}
static void cloud_changed(mi355ndt_handle* h, bool tgt, int pair, size_t count, bool has_intensity = false) { cloud_changed(h, tgt, pair, 1, &count, has_intensity); }
// the intensity row of a slot of the engine's own batch that carries one (else null)
static float* slot_intensity_row(mi355ndt_handle* h, bool tgt, int pair) {
  const std::vector<unsigned char>& has_i = tgt ? h->tgt_has_i : h->src_has_i;
  DevBuf<float>& plane = tgt ? h->d_tgt_i : h->d_src_i;
  if ((size_t)pair >= has_i.size() || !has_i[(size_t)pair] || !plane || (tgt ? h->d_tgt != h->d_tgt_own : h->d_src != h->d_src_own)) return nullptr;
  return plane + (size_t)pair * (tgt ? h->tgt_pitch : h->src_pitch);
}
// The slots of a side hold nothing any more (their rows were re-allocated, the batch got another shape, an alias ended).
static void clouds_reset(mi355ndt_handle* h, bool tgt, bool src) {
  std::lock_guard<std::mutex> lk(h->up_mtx);
  if (tgt) { std::fill(h->h_tgt_cnt.begin(), h->h_tgt_cnt.end(), 0); h->tgt_has_i.assign(h->h_tgt_cnt.size(), 0); h->have_target = false; h->built.valid = false; }
  if (src) { std::fill(h->h_src_cnt.begin(), h->h_src_cnt.end(), 0); h->src_has_i.assign(h->h_src_cnt.size(), 0); h->have_source = false; }
}
// May an align of this configuration be ONE persistent launch (ndt_async.hpp)?  Asked by mi355ndt_batch_align and by mi355ndt_stream_begin.
static bool async_served(const mi355ndt_handle* h) { return h->async_align && !mt_is_live(h->prm) && !is_pca_kd(h->prm) && model_leaves_rounds(h->pose_model, h->ndt_class, h->ground_class); }
// algorithmic bytes of sweeping `points` points: every point is streamed (12 B) and probes K table words
static double sweep_alg_bytes(double points, int K) { return points * (12.0 + 4.0 * K); }
// resident workgroup slots of a sweep launch or a persistent launch; `fast`: the tolerance arithmetic's kernels serve it.  (Callers decide
// `fast` by sweep_ord(...) == 2 or by fast_served(h); the two differ before the fast records are built: ndt_host_sweep.hpp, sweep_ord.)
// `lean`: a persistent launch of the lean item body (async_lean, ndt_host_sweep.hpp): three slots per CU.
static int launch_slots(const mi355ndt_handle* h, const SweepConst& sc, bool fast, bool lean = false) { return h->n_cu * sweep_wpe(sc.K, fast, lean); }
