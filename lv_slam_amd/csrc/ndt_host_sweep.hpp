// ndt_host_sweep.hpp -- what every align path launches: the align workspace and the SweepConst of a configuration, the lookup from a run-time
// tag to a kernel instantiation, launch_sweep, launch_hessian, and the one persistent launch (launch_async).
#pragma once

// ---- which kernel serves ------------------------------------------------------------------------
// The table of the instantiations of k_sweep / k_sweep_pca_kd / k_align_async (host-only, shared with the tests): a run-time tag is looked up
// among its rows, and a row alone names a kernel.  nullptr: no such instantiation.
#include "ndt_sweep_exists.hpp"
static_assert(SWEEP_IT_BATCH == 8, "the IT column of the table's batch-mode rows");
using SweepKernel = void (*) NDT_SWEEP_ARGS_T;
using KdKernel = void (*) NDT_KD_ARGS_T;
static SweepKernel sweep_kernel(const SweepTag& t) {
#define NDT_ROW(PCA, K, IT, ORD, PM, GATE) if (same(t, SweepTag{PCA, K, IT, ORD, PM, GATE})) return NDT_SWEEP_TAG(PCA, K, IT, ORD, PM, GATE);
  NDT_SWEEP_ROWS(NDT_ROW)
#undef NDT_ROW
  return nullptr;
}
static KdKernel kd_kernel(int ord) {
#define NDT_ROW(ORD) if (ord == ORD) return NDT_KD_TAG(ORD);
  NDT_KD_ROWS(NDT_ROW)
#undef NDT_ROW
  return nullptr;
}

// ---- two or three waves per SIMD in a persistent launch (MI355NDT_OPT_SWEEP_WAVES) ----------------
// Decided once per launch, on the host (a stream: by the batch the launch starts, stream_launch): ndt_sweep_waves.hpp has the rule and where its threshold comes from.
// `ord`: the arithmetic of the launch's sweeps (sweep_ord); `tgt_pts`: the largest target of the batch.
static_assert(sizeof(VoxelRec) == LEAN_REC_BYTES, "the record the estimate counts");
static bool async_lean(const mi355ndt_handle* h, const SweepConst& sc, int ord, size_t tgt_pts) {
  return async_served(h) && lean_exists(sc.pca != 0, sc.K, ord) && sweep_waves_choice(h->sweep_waves, h->prm, ord, tgt_pts) == 3;
}
// stream mode: the slots a lean launch leaves to the next batch's build -- of 768, a third of a CU each (mi355ndt_stream_begin has the sweep)
constexpr int LEAN_RESERVE_WG = 96;

// ---- sweeps -----------------------------------------------------------------------------------
static int prep_align_ws(mi355ndt_handle* h) {
  const int B = h->n_pairs;
  int maxn = 0;
  for (int b = 0; b < B; b++) maxn = std::max(maxn, h->h_src_cnt[b]);
  h->chunks_per_pair = std::max(1, (maxn + CHUNK_PTS - 1) / CHUNK_PTS);
  // latency mode (mi355ndt_set_latency_mode): fine work items for small batches, where the 512-point items of the batch mode leave
  // most of the GPU idle.  Served by the DIRECT1 / DIRECT7 instantiations; the live More-Thuente case keeps the batch kernels.
  {
    const bool fine_served = sweep_exists(false, neighbor_K(h->prm.neighbor_mode), 0, h->fine_tiles);
    // "small": fewer batch-mode items than two per resident wave; a sequence run sweeps ONE pair at a time whatever the number of frames
    const bool small = h->seq_running || (long long)B * h->chunks_per_pair * QUARTERS < 4LL * h->n_cu * WAVES;
    h->fine_it = (h->latency_mode && fine_served && !mt_is_live(h->prm) && small && model_leaves_rounds(h->pose_model, h->ndt_class, h->ground_class)) ? h->fine_tiles : 0;
  }
  if (eff_model(h) == POSE_MODEL_EULER) HIPCHK(h, h->d_euler_rows.reserve((size_t)B * EULER_ROW_WORDS));
  if (h->ndt_class == NDT_CLASS_PCL) HIPCHK(h, h->d_pcl_rows.reserve((size_t)B * EULER_ROW_WORDS));
  if (h->fine_it) {
    const int item_pts = h->fine_it * 64;
    h->pts_per_chunk = 4 * item_pts;                                   // a block of the fine sweep = four items = one chunk, stored as ONE row
    h->rows_per_pair = std::max(1, (maxn + h->pts_per_chunk - 1) / h->pts_per_chunk);
    h->items_per_pair = 4 * h->rows_per_pair;
  } else {
    h->rows_per_pair = h->chunks_per_pair * QUARTERS;
    h->items_per_pair = h->rows_per_pair;
    h->pts_per_chunk = CHUNK_PTS;
  }
  size_t need = (size_t)B * std::max(h->rows_per_pair, h->chunks_per_pair * QUARTERS) * NACC;   // (the parity hooks may fall back to batch-mode rows)
  HIPCHK(h, h->d_partials.reserve(need));
  if (h->up_src_cnt.size() != (size_t)B || !std::equal(h->up_src_cnt.begin(), h->up_src_cnt.end(), h->h_src_cnt.begin())) {
    HIPCHK(h, hipMemcpyAsync(h->d_src_cnt, h->h_src_cnt.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->up_src_cnt.assign(h->h_src_cnt.begin(), h->h_src_cnt.begin() + B);
  }
  return MI355NDT_OK;
}

static void make_sweep_const(const mi355ndt_handle* h, SweepConst& sc) {
  double d1, d2;
  gauss_constants(h->prm, d1, d2);
  sc.d1 = d1;
  sc.d2f = (float)d2;                        // impl2:578
  sc.pca = h->prm.variant == MI355NDT_VARIANT_PCA;
  // the lookup divides by the GRID's leaf size (voxel_grid_covariance_omp_impl.hpp:379-381), which is resolution_ except after a setResolution
  // that found no source and therefore left the grid alone (ndt_omp.h:126-136); the Gauss constants and the kd radius follow resolution_
  const float leaf = (h->built.valid && h->built.leaf > 0.f) ? h->built.leaf : h->prm.resolution;
  { int ex; float mant = std::frexp(leaf, &ex); sc.leaf_pow2 = (mant == 0.5f) && ex > -100 && ex < 100; sc.inv_leaf = 1.0f / leaf; }
  sc.kd_r2 = (float)((double)h->prm.resolution * (double)h->prm.resolution);   // KdTreeFLANN::radiusSearch: float(radius * radius)
  build_offsets(class_neighbor_mode(h->ndt_class, h->prm.neighbor_mode), sc);   // (class 1: always the radius search)
  sc.dyn_shift = h->dyn_shift >= 0 ? h->dyn_shift : (sc.K == 1 ? 3 : 2);
  sc.host_flags = nullptr;
  sc.seq_no = 0;
  sc.rebase_block = 0;
  sc.d1f = (float)d1;
  sc.kq = (float)(-0.5 * (double)sc.d2f * 1.4426950408889634);   // exp(-d2 q / 2) = 2^(kq q)
  sc.euler_rows = euler_rows_of(h);
  sc.pcl_rows = pcl_rows_of(h);
  sc.icov64 = h->d_icov64.p;
  sc.d2 = d2;
  sc.leaf_class = ground_gated(h->ground_class) ? h->d_leaf_class.p : nullptr;
  sc.gate_code = ground_gated(h->ground_class) ? h->ground_class : 0;          // (GROUND_CLASS_HORIZONTAL / _VERTICAL are LEAF_CLASS_HORIZONTAL / _VERTICAL)
}

// The arithmetic a sweep runs in: 2 = tolerance arithmetic (MI355NDT_OPT_ARITH = 1; instantiated for DIRECT1 / DIRECT7 with the dead More-Thuente
// loop -- every configuration lv_slam ships; the other searches and the live line search keep the exact kernels), else the f32 sum order.
static int sweep_ord(const mi355ndt_handle* h, const SweepConst& sc) {
  if (h->ndt_class == NDT_CLASS_PCL) return 0;    // (no three-term f32 sum in the f64 evaluation: MI355NDT_OPT_F32_SUM_ORDER moves no word)
  // (a stream's parent handle owns no grids: its contexts' engines build them, with the option as it stood at mi355ndt_stream_begin)
  if (fast_served(h) && (h->built.made.recs_fast || h->ss)) return 2;
  return h->f32_sum_order;
}
static const VoxelRec* sweep_recs(const mi355ndt_handle* h, const SweepConst& sc) {
  return sweep_ord(h, sc) == 2 ? reinterpret_cast<const VoxelRec*>(h->d_recs_fast.p) : h->d_recs;
}

// The three families beside the SE(3) sweeps have rows with ORD = 0 / 1 alone, so wherever one of them launches, sweep_recs(h, sc) is h->d_recs
// (the tolerance arithmetic's records go to ORD = 2 only): launch_sweep passes sweep_recs to every kernel of the table.
#define NDT_ROW(PCA, K, IT, ORD, PM, GATE) && !((PM != 0 || GATE) && ORD == 2)
static_assert(true NDT_SWEEP_ROWS(NDT_ROW), "a row of the Euler model, of PCL's class or of the gated sweep reads the tolerance arithmetic's records");
#undef NDT_ROW

static int launch_sweep(mi355ndt_handle* h, const SweepConst& sc, int max_pairs = -1) {
  // persistent waves: SWEEP_WPE workgroups per CU pull (pair, chunk, quarter) items until the per-XCD queues are dry
  const int ord = sweep_ord(h, sc);
  dim3 grid((unsigned)launch_slots(h, sc, ord == 2));
  if (h->prof) HIPCHK(h, ev_begin(h, h->ev_sweep));
  SweepCtl *ctl = h->d_ctl + h->ctl_idx, *ctl_next = h->d_ctl + (h->ctl_idx ^ 1);
  if (h->fine_it) {                              // latency mode: items dealt statically over the whole grid, sized to the work there can be
    const long long items = (long long)(max_pairs > 0 ? max_pairs : h->n_pairs) * h->items_per_pair;
    grid.x = (unsigned)std::max(1LL, std::min((long long)grid.x, (items + WAVES - 1) / WAVES));
    if (sc.rebase_block) grid.x += 1;              // + the workgroup that computes the next update's re-basing instead of sweeping
  }
  // the family, what it needs besides its kernel, and what it says when it is not served
  SweepTag t{sc.pca != 0, sc.K, h->fine_it ? h->fine_it : SWEEP_IT_BATCH, ord, 0, false};
  bool ready = true;
  const char* why = "no sweep kernel serves this configuration";
  if (h->ndt_class == NDT_CLASS_PCL) {             // pcl::NormalDistributionsTransform: one kernel -- the radius search, the f64 evaluation
    t.pm = 2;
    ready = !sc.pca && !h->fine_it && sc.pcl_rows && sc.icov64 && h->built.made.icov64 && h->built.made.cent;
    why = "no sweep kernel serves this configuration under MI355NDT_OPT_NDT_CLASS = 1";
  } else if (h->pose_model == POSE_MODEL_EULER) {
    t.pm = 1;
    ready = !sc.pca && !h->fine_it && sc.euler_rows;
    why = "no sweep kernel serves this configuration under MI355NDT_OPT_POSE_MODEL = 1";
  } else if (ground_gated(h->ground_class)) {      // pclomp_ground, flag_class 1 / 2: the gated probe stage (class 3 is the plain ndt_omp sweep)
    t.gate = true;
    ready = !sc.pca && !h->fine_it && sc.leaf_class && h->built.made.leaf_class && (sc.gate_code == 1 || sc.gate_code == 2);
    why = "no sweep kernel serves this configuration under MI355NDT_OPT_GROUND_CLASS = 1 / 2";
  }
  if (t.pm == 0 && !t.gate && !h->fine_it && sc.pca && sc.K == 27) {     // ndt_pca + KDTREE: order-dependent weights, the literal kernel (ndt_sweep_kd.hpp)
    const KdKernel kd = kd_kernel(ord);
    if (!kd) { h->err = why; return MI355NDT_ERR_UNSUPPORTED; }
    const dim3 kdgrid((unsigned)h->chunks_per_pair, (unsigned)h->n_pairs);
    kd<<<kdgrid, SWEEP_THREADS, 0, h->stream>>>(h->d_src, h->src_pitch, h->d_state, h->d_grid, h->d_words, h->d_recs, h->d_cent, h->d_kdw, h->d_partials,
                                                h->chunks_per_pair, h->d_active_list, ctl, ctl_next, sc);
  } else {
    // (the f32 sum order is a template parameter: the alternative order costs no instruction, only a second set of instantiations)
    const SweepKernel kern = ready ? sweep_kernel(t) : nullptr;
    if (!kern) { h->err = why; return MI355NDT_ERR_UNSUPPORTED; }
    kern<<<grid, SWEEP_THREADS, 0, h->stream>>>(h->d_src, h->src_pitch, h->d_state, h->d_grid, h->d_words, sweep_recs(h, sc), h->d_partials, h->items_per_pair,
                                                h->d_active_list, ctl, ctl_next, sc, h->d_cent, h->d_grid_of_use);
  }
  h->ctl_idx ^= 1;                                // the block this sweep zeroed is the one the next update fills
  if (h->prof) HIPCHK(h, ev_end(h, h->ev_sweep));
  return MI355NDT_OK;
}

static void launch_hessian(mi355ndt_handle* h, const SweepConst& sc) {
  double gc[3] = {0, 0, 0};
  gauss_constants(h->prm, gc[0], gc[1]);
  k_hessian<<<dim3((unsigned)h->chunks_per_pair, (unsigned)h->n_pairs), HESS_THREADS, 0, h->stream>>>(
      h->d_src, h->src_pitch, h->d_state, h->d_grid, h->d_words, h->d_recs, h->d_icov64, h->d_cent, h->d_partials, h->chunks_per_pair,
      gc[0], gc[1], sc.kd_r2, sc.leaf_pow2, sc.inv_leaf);
}

// One persistent launch for the whole batch align (ndt_async.hpp): served for the DIRECT / KDTREE sweeps of k_sweep with the dead
// More-Thuente loop -- every configuration lv_slam ships.  Returns MI355NDT_ERR_UNSUPPORTED when the launch cannot be made resident
// (the caller then takes the lockstep path).

// What one persistent launch needs besides the engine's parameters: the context table (one context: the synchronous batch align; several:
// the stream mode), the NEW context's arrays for the prepare kernel, the rings and the control blocks.
struct AsyncLaunch {
  AsyncTab tab;
  int new_ci = 0, n_new = 0;                       // context and number of the pairs that START in this launch (0: only carried pairs)
  PairState* st_new = nullptr; const float* guess_new = nullptr; const int* src_cnt_new = nullptr; const GridDesc* gd_new = nullptr; unsigned* arrived_new = nullptr;
  int* active_list = nullptr; SweepCtl* sweep_ctl = nullptr; unsigned* done_new = nullptr; PoseRecord* pose_new = nullptr; int pose_cap = 0;
  AsyncTab* tab_dev = nullptr; int* ring = nullptr; int ring_cap = 0; AsyncCtl* ctl = nullptr; const AsyncCtl* prev = nullptr;
  int items_per_pair = 0, stop_thresh = 0; unsigned debug_abort_pos = 0xFFFFFFFFu, debug_ring_mask = 0xFFu;
  unsigned long long* stamp_end = nullptr;       // stream mode + profiling: where k_async_prepare stamps the end of the build in front of it
  int claim_items = 1;                           // DIRECT7 items per claimed position (DIRECT1: always ASYNC_CLAIM(1) = 2; ndt_async.hpp)
  int reserve_wg = 0;
  bool lean = false;                             // the lean item body, three waves per SIMD (async_lean: the caller decides, per launch)
  hipEvent_t ev_prepared = nullptr;              // stream mode, build beside the launch: recorded between the prepare kernel and the persistent launch
};
#define NDT_CTX_ARGS(i) L.tab.c[i].src, L.tab.c[i].pitch, L.tab.c[i].st, L.tab.c[i].gd, L.tab.c[i].words, L.tab.c[i].recs, L.tab.c[i].partials, L.tab.c[i].src_cnt, \
                        L.tab.c[i].arrived, L.tab.c[i].cent
template <bool PCA, int K, int ORD, bool LEAN>
static int launch_async_t(mi355ndt_handle* h, const SweepConst& sc, const AsyncLaunch& L) {
  auto kern = NDT_ALIGN_TAG(PCA, K, ORD, LEAN);
  // (asked once per instantiation and device: the query sits between the prepare kernel and the launch, on the host's critical path)
  // (engines on several host threads come through here at once: the cached answer is an atomic, the query writes into a local)
  static std::atomic<int> per_cu_of_device[64];
  int per_cu = per_cu_of_device[h->device & 63].load(std::memory_order_relaxed);
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, SWEEP_THREADS, 0) != hipSuccess) { (void)hipGetLastError(); return MI355NDT_ERR_UNSUPPORTED; }
    per_cu_of_device[h->device & 63].store(per_cu, std::memory_order_relaxed);
  }
  const int slots = launch_slots(h, sc, ORD == 2, LEAN);
  // Workgroup L serves ring L % 8 first, and the launch is sized to be resident as a whole.  Residency is no condition of correctness:
  // positions are claimed, a waiting wave serves the published positions of OTHER rings too (ndt_async.hpp: an XCD that holds no workgroup
  // of this launch -- another engine's launch fills it -- leaves no ticket unserved), a workgroup that starts late finds the launch over
  // or joins in; a launch that cannot progress all the same ends itself (bounded polls) and the caller falls back to the rounds.
  if (per_cu * h->n_cu < slots || slots < 8) return MI355NDT_ERR_UNSUPPORTED;
  // (stream mode may withhold some workgroups so that the next batch's target build, on a stream of its own, finds wave slots
  //  beside this launch: L.reserve_wg, a multiple of 8 so that every ring loses the same number of waves)
  dim3 grid((unsigned)std::max(8, slots - L.reserve_wg));
  kern<<<grid, SWEEP_THREADS, 0, h->stream>>>(L.tab_dev, L.items_per_pair, L.ring, L.ring_cap, L.ctl, sc, h->prof ? h->d_hits : nullptr,
                                             h->prm.step_size, h->prm.trans_epsilon, h->prm.max_iterations, L.stop_thresh, L.debug_abort_pos, L.debug_ring_mask, L.claim_items,
                                             NDT_CTX_ARGS(0), NDT_CTX_ARGS(1), NDT_CTX_ARGS(2), NDT_CTX_ARGS(3));
  h->last_async_wpe = SweepTune<PCA, K, ORD, LEAN>::WPE; h->last_async_grid = (int)grid.x;
  return MI355NDT_OK;
}
// prepare kernel + the persistent launch on the engine's stream (HIP events around the launch when profiling)
static int launch_async(mi355ndt_handle* h, const SweepConst& sc, const AsyncLaunch& L) {
  hipStream_t s = h->stream;
  {
    const size_t n = std::max(std::max(std::max((size_t)8 * L.ring_cap, (size_t)L.n_new * ASYNC_ARR_STRIDE), sizeof(AsyncCtl) / sizeof(unsigned)), (size_t)L.pose_cap);
    k_async_prepare<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(L.tab, L.tab_dev, L.new_ci, L.n_new, L.st_new, L.guess_new, L.src_cnt_new, L.gd_new, L.arrived_new,
                                                               L.active_list, L.sweep_ctl, L.ring, L.ring_cap, L.ctl, L.prev, L.done_new, L.pose_new, L.pose_cap, L.stamp_end);
    if (L.ev_prepared) HIPCHK(h, hipEventRecord(L.ev_prepared, s));
  }
  if (h->prof) HIPCHK(h, ev_begin(h, h->ev_sweep));
  // (a one-launch align sweeps batch-mode items; ORD as the sweeps of this engine have it: sweep_ord; the lean body when the launch asks for
  // it and the table has the row)
  const int rc = [&] {
    AlignTag t{sc.pca != 0, sc.K, sweep_ord(h, sc), false};
    t.lean = L.lean && lean_exists(t.pca, t.K, t.ord);
#define NDT_ROW(PCA, K, ORD, LEAN) if (same(t, AlignTag{PCA, K, ORD, LEAN})) return launch_async_t<PCA, K, ORD, LEAN>(h, sc, L);
    NDT_ALIGN_ROWS(NDT_ROW)
#undef NDT_ROW
    return (int)MI355NDT_ERR_UNSUPPORTED;
  }();
  if (h->prof) HIPCHK(h, ev_end(h, h->ev_sweep));
  return rc;
}
// ring slots a launch over at most `pairs` pairs can need: every pair publishes at most max_iterations + 3 tickets.
// 0: too many for a sane allocation (the caller takes the round-based path, which needs no ring)
static int async_ring_cap(const mi355ndt_handle* h, long long pairs) {
  const long long cap = (pairs * ((long long)h->prm.max_iterations + 4) + 7) / 8 + 1;
  return cap > (1LL << 26) ? 0 : (int)cap;        // 8 rings x 2^26 words = 2 GB: beyond that the rounds are the right tool anyway
}
static void fill_async_ctx(const mi355ndt_handle* e, AsyncCtx& c) {
  SweepConst sc;
  make_sweep_const(e, sc);
  c.src = e->d_src; c.pitch = e->src_pitch; c.st = e->d_state; c.gd = e->d_grid; c.words = e->d_words; c.recs = sweep_recs(e, sc); c.cent = e->d_cent;
  c.partials = e->d_partials; c.src_cnt = e->d_src_cnt; c.arrived = e->d_arrived; c.results = e->d_results; c.n_done = nullptr; c.must_finish = 1; c.pose = nullptr; c.pose_base = 0; c.pose_stride = 0; c.score_only = e->score_only_last;
}
