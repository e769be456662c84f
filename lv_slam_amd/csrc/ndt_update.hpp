// ndt_update.hpp -- the update between two sweeps of a pair: the fixed-order reduction of its partial rows (one statement of the tree for the
// block form and the one-wave form), the pieces around it (sums into the state, state to LDS and back), the block-level update body of
// k_update and k_seq_update (ndt_sequence.hpp), and the pose set-up kernels.  The Newton control itself is ndt_newton.hpp; the one-launch
// align builds its updater from the same pieces (async_update, ndt_async.hpp).
#pragma once
#include "ndt_types.hpp"
#include "ndt_math.hpp"
#include "ndt_newton.hpp"
#include "ndt_sweep.hpp"

// p = SE3(R,t).log(); first sweep moves the cloud by the caller's f32 guess itself (impl2:102-129)
// euler_rows: non-null = MI355NDT_OPT_POSE_MODEL 1 (impl.hpp:95-119), the pairs' row slots
NDT_KERNEL void k_init_state(PairState* st, const float* __restrict__ guess_cm, const int* __restrict__ src_cnt,
                             const GridDesc* __restrict__ gd, int n_pairs, int* active_list, SweepCtl* ctl, float* euler_rows,
                             double* pcl_rows /* non-null: MI355NDT_OPT_NDT_CLASS 1, the rows as doubles */) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_pairs) return;
  active_list[b] = b;                            // the first sweep covers every pair
  if (b == 0) ctl->n_active = n_pairs;
  if (euler_rows) init_pair_state<1>(st[b], guess_cm + (size_t)b * 16, src_cnt[b], gd[b].status, euler_rows + (size_t)b * EULER_ROW_WORDS,
                                     pcl_rows ? pcl_rows + (size_t)b * EULER_ROW_WORDS : nullptr);
  else init_pair_state(st[b], guess_cm + (size_t)b * 16, src_cnt[b], gd[b].status);
}

// explicit sweep pose (parity hooks)
NDT_KERNEL void k_set_pose(PairState* st, int b, const float* __restrict__ T_cm, const float* __restrict__ Rj, const int* __restrict__ src_cnt,
                           const GridDesc* __restrict__ gd, int* active_list, SweepCtl* ctl) {
  PairState& S = st[b];
  active_list[0] = b; ctl->n_active = 1;
  for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) S.T[r * 4 + c] = T_cm[c * 4 + r];
  for (int a = 0; a < 9; a++) S.Rj[a] = Rj[a];
  S.phase = PH_SWEEP0; S.n_src = src_cnt[b]; S.grid_status = gd[b].status; S.it = 0; S.sweeps = 1; S.last_sweep = 0;
}
// euler_rows: non-null = MI355NDT_OPT_POSE_MODEL 1, p = [t; roll pitch yaw]: the cloud is moved by convertTransform(p), the rows are taken from p
NDT_KERNEL void k_set_pose_p(PairState* st, int b, const double* __restrict__ p, const int* __restrict__ src_cnt, const GridDesc* __restrict__ gd,
                             int* active_list, SweepCtl* ctl, int for_hessian, float* euler_rows, double* pcl_rows) {
  PairState& S = st[b];
  active_list[0] = b; ctl->n_active = 1;
  double pp[6];
  for (int a = 0; a < 6; a++) { pp[a] = p[a]; S.xt[a] = p[a]; }
  if (euler_rows) pose_to_sweep<1>(pp, S, euler_rows + (size_t)b * EULER_ROW_WORDS, pcl_rows ? pcl_rows + (size_t)b * EULER_ROW_WORDS : nullptr);
  else pose_to_sweep<0>(pp, S, nullptr);
  S.phase = for_hessian ? PH_HESS : PH_SWEEP0; S.n_src = src_cnt[b]; S.grid_status = gd[b].status; S.it = 0; S.sweeps = 1; S.last_sweep = 0;
}

// ---- fixed-order reduction of one pair's partial rows ------------------------------------------------------------------
// A pair's sweep leaves one 44-double row per work item (score, g[6], H[36], hits).  Four consecutive rows form a CHUNK,
// ((r0 + r1) + r2) + r3 (impl2:298-302 adds per-thread sums in a fixed order; so does this).  Eight consecutive chunks form a
// GROUP, added in chunk order.  Group k belongs to wave k % UPD_WAVES (= 4) of the block, which adds its groups in ascending order;
// the four wave sums then add up in wave order.  (Four waves = one per SIMD: the Newton step wants 300+ VGPRs.)  The tree is a function of the number of chunks alone -- never of the batch,
// the launch geometry or which wave ran an item -- so batched and single runs of a pair stay bit-identical; up to eight chunks
// (16,384 points) it is the plain sequential sum.
// Every route states the tree through the three functions below -- chunk_sum, group_sum, wave_sums_total -- and walk_groups; the routes
// differ only in which groups a wave walks and how many it keeps in flight (tests/test_row_tree_gpu.py holds all of them to the tree
// written out in numpy).
#define UPD_WAVES   4
#define UPD_THREADS (64 * UPD_WAVES)
#define GROUP_CHUNKS 8
// SC1: the rows were written by other workgroups of THIS launch (persistent kernels): read them with agent-scope (L1-bypassing) loads.
template <bool SC1>
__device__ __forceinline__ double ld_row(const double* p) {
  if (SC1) return __longlong_as_double((long long)__hip_atomic_load((const gu64*)reinterpret_cast<const unsigned long long*>(p), RLX_AGENT));
  return *p;
}
// RPC = stored rows per chunk: 4, or 1 where the rows are chunk sums already (latency mode: the sweep's blocks add the four rows of a chunk themselves)
template <int RPC>
__device__ __forceinline__ double chunk_sum(const double r[RPC]) {
  static_assert(RPC == 1 || RPC == 4, "a chunk is stored as its four rows or as their sum");
  if constexpr (RPC == 4) return ((r[0] + r[1]) + r[2]) + r[3];
  else return r[0];
}
// group g over the chunks that exist (FULL: all eight do); q = its rows as walk_batch loaded them
template <int RPC, bool FULL>
__device__ __forceinline__ double group_sum(const double q[GROUP_CHUNKS][RPC], const int g, const int nchunks) {
  double gs = 0.0;
#pragma unroll
  for (int u = 0; u < GROUP_CHUNKS; u++) if (FULL || g * GROUP_CHUNKS + u < nchunks) gs += chunk_sum<RPC>(q[u]);
  return gs;
}
__device__ __forceinline__ double wave_sums_total(const double a0, const double a1, const double a2, const double a3) {
  double v = 0.0;
  v += a0; v += a1; v += a2; v += a3;
  return v;
}
// One lane's column `P` of the rows: walks groups first, first + step, ... with the loads of NF of them in flight together, and adds the
// j-th group of the walk into acc[j % NA] -- a wave-uniform choice between NA compile-time cases, never a run-time register index.
//   block form:    wave w walks w, w + UPD_WAVES, ... into its one accumulator (NA = 1); all 32 loads of a group in flight, or with chunk
//                  rows those of four groups (a 65,536-point pair in latency mode has 128 chunk rows = 16 groups = four per wave: one memory
//                  round trip; the reduction of a 131,072-point pair in batch mode -- 256 rows -- is two round trips per wave instead of eight on one wave);
//   one-wave form: walks 0, 1, 2, ... into the four accumulators that stand for the block's waves (NA = UPD_WAVES, step = 1).
// One batch of the walk: groups g0, g0 + step, ... (NF of them), the j0-th and following of the walk.  FULL: every chunk of the batch exists,
// so the loads are unconditional straight-line code; otherwise each is guarded by the chunk count (a scalar branch per load: the one-launch
// updater lost 2 % of a config-5 DIRECT1 launch when its full batches went that way too, docs/experiments.md 10l).
template <int RPC, bool SC1, int NF, int NA, bool FULL>
__device__ __forceinline__ void walk_batch(const double* P, const int nchunks, const int g0, const int step, const int j0, double (&acc)[NA]) {
  double q[NF][GROUP_CHUNKS][RPC];
#pragma unroll
  for (int f = 0; f < NF; f++)
#pragma unroll
    for (int u = 0; u < GROUP_CHUNKS; u++)
#pragma unroll
      for (int k = 0; k < RPC; k++) {
        const int c = (g0 + f * step) * GROUP_CHUNKS + u;
        q[f][u][k] = (FULL || c < nchunks) ? ld_row<SC1>(P + ((size_t)c * RPC + k) * NACC) : 0.0;
      }
#pragma unroll
  for (int f = 0; f < NF; f++) {
    const int g = g0 + f * step;
    if (!FULL && g * GROUP_CHUNKS >= nchunks) break;
    const double gs = group_sum<RPC, FULL>(q[f], g, nchunks);
#pragma unroll
    for (int k = 0; k < NA; k++) if ((j0 + f) % NA == k) acc[k] += gs;
  }
}
template <int RPC, bool SC1, int NF, int NA>
__device__ __forceinline__ void walk_groups(const double* P, const int nchunks, const int first, const int step, double (&acc)[NA]) {
#pragma unroll 1
  for (int j0 = 0, g0 = first; g0 * GROUP_CHUNKS < nchunks; j0 += NF, g0 += NF * step) {
    if ((g0 + (NF - 1) * step + 1) * GROUP_CHUNKS <= nchunks) walk_batch<RPC, SC1, NF, NA, true>(P, nchunks, g0, step, j0, acc);
    else walk_batch<RPC, SC1, NF, NA, false>(P, nchunks, g0, step, j0, acc);
  }
}

// The block form: lane < NACC of every wave owns a column; returns the column's sum on wave 0.  `take` = false: the lane's column is not
// wanted (its sum is 0).  (The barrier inside also publishes whatever the block wrote to LDS before the call.)
template <bool SC1 = false>
__device__ __forceinline__ double reduce_pair_rows(const double* __restrict__ rows, int nchunks, bool take, double (*sm)[NACC], bool chunk_rows = false) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane < NACC) {
    double acc[1] = {0.0};
    if (take) {
      if (chunk_rows) walk_groups<1, SC1, 4, 1>(rows + lane, nchunks, w, UPD_WAVES, acc);
      else walk_groups<4, SC1, 1, 1>(rows + lane, nchunks, w, UPD_WAVES, acc);
    }
    sm[w][lane] = acc[0];
  }
  __syncthreads();
  double v = 0.0;
  if (w == 0 && lane < NACC) v = wave_sums_total(sm[0][lane], sm[1][lane], sm[2][lane], sm[3][lane]);
  static_assert(UPD_WAVES == 4, "four wave sums");
  return v;
}

// ---- the pieces around the tree ------------------------------------------------------------------------------------------
// Column `lane` of the row sums -> its field of the state.  h_only: the computeHessian pass fills H alone; score_hits_only: a sweep marked
// as the pair's last (PairState::last_sweep) left rows that carry the score and the hit count alone -- the other columns are stale.
// hits_total (may be null, profiling): [0] += hits, [1] counts the score-only sums.
enum { COL_SCORE = 0, COL_H = 7, COL_HITS = NACC - 1 };
__device__ __forceinline__ bool sums_live(const int lane, const bool h_only, const bool score_hits_only) {
  if (h_only) return lane >= COL_H && lane < COL_HITS;
  if (score_hits_only) return lane == COL_SCORE || lane == COL_HITS;
  return lane < NACC;
}
// MI355NDT_OPT_GROUND_CLASS (ground = 1 / 2 / 3): what pclomp_ground does to the sums of a sweep.  Every hit is evaluated twice into the point's
// gradient and Hessian and once into its score (ndt_ground_impl.hpp:519, 522), so g and H are twice the sums over the same hits -- exact in f64 --
// and the score is as summed; then class 1 zeroes rows and columns 0, 1, 5 of H and g(0), g(1), g(5), class 2 rows and columns 2, 3, 4
// (:554-567); class 3 (flag_class 0) masks nothing.  A masked entry is +0.0 whatever was summed.
__device__ __forceinline__ double ground_sum(const int lane, const double v, const int ground) {
  if (ground == 0 || lane < 1 || lane >= COL_HITS) return v;
  const int masked = ground == 1 ? 0x23 : (ground == 2 ? 0x1C : 0);               // bit a: pose component a is held
  const int i = lane < COL_H ? lane - 1 : (lane - COL_H) / 6, j = lane < COL_H ? lane - 1 : (lane - COL_H) % 6;
  return (((masked >> i) | (masked >> j)) & 1) ? 0.0 : 2.0 * v;
}
__device__ __forceinline__ void store_sums(PairState& S, const int lane, const double v_in, const bool h_only, const bool score_hits_only, unsigned long long* hits_total,
                                           const int ground = 0) {
  if (!sums_live(lane, h_only, score_hits_only)) return;
  const double v = ground_sum(lane, v_in, ground);
  if (lane == 0) S.score = v;
  else if (lane < 7) S.g[lane - 1] = v;
  else if (lane < 43) S.H[lane - 7] = v;
  else {
    S.hits = (long long)v;
    if (hits_total) { atomicAdd(hits_total, (unsigned long long)v); if (score_hits_only) atomicAdd(hits_total + 1, 1ull); }
  }
}

// The pair's state lives in LDS for the duration of an update: the Newton step reads and writes some sixty of its fields one after the
// other, and through a global reference every first touch of a line was a memory round trip of its own (rounds 3-4, latency mode: 11.5 us
// per update, most of it such waits).  `n` threads copy, `tid` = this thread's index among them.  SC1: agent-scope accesses (the state
// crosses workgroups inside one launch: L1-bypassing loads, write-through stores).
constexpr int PAIR_STATE_WORDS = (int)(sizeof(PairState) / 8);
static_assert(sizeof(PairState) % 8 == 0, "PairState travels as 8-byte words");
template <bool SC1>
__device__ __forceinline__ void state_to_lds(PairState& L, const PairState* G, const int tid, const int n) {
  unsigned long long* sl = reinterpret_cast<unsigned long long*>(&L);
  const unsigned long long* sg = reinterpret_cast<const unsigned long long*>(G);
  for (int i = tid; i < PAIR_STATE_WORDS; i += n) sl[i] = SC1 ? __hip_atomic_load((const gu64*)sg + i, RLX_AGENT) : sg[i];
}
template <bool SC1>
__device__ __forceinline__ void state_from_lds(PairState* G, const PairState& L, const int tid, const int n) {
  const unsigned long long* sl = reinterpret_cast<const unsigned long long*>(&L);
  unsigned long long* sg = reinterpret_cast<unsigned long long*>(G);
  for (int i = tid; i < PAIR_STATE_WORDS; i += n) {
    if (SC1) __hip_atomic_store((gu64*)sg + i, sl[i], RLX_AGENT);
    else sg[i] = sl[i];
  }
}
// what one lane of a wave wrote to LDS is there for the other lanes of that wave
__device__ __forceinline__ void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// ---- the block-level update -------------------------------------------------------------------------------------------
// One block of UPD_WAVES waves and one pair: state into LDS, the row tree, the sums into the state, then the solve on the second wave
// next to newton_update on the first.  Returns newton_update's code on wave 0 (valid on its lane 0; NEWTON_DONE too where reduce_only
// skipped the step), whose caller acts on it and sends the state back (state_from_lds); UPD_EXIT on every thread that is done.
//   STATE_FIRST: the point count and the phase come out of the state (k_update), at the price of a barrier before the rows are requested;
//   otherwise the caller knows n_src (latency mode: the run position says it) and state and rows travel together.
//   `pts_per_chunk` = points covered by one chunk = four consecutive rows (CHUNK_PTS in batch mode) or, with `chunk_rows`, by one stored row.
//   tl (may be null): latency mode's timeline, slots 9 (state + rows) and 13 / 14 (wave 1: solve); tools/seq_run.py.
enum { UPD_EXIT = -1 };
//   PM / pose_rows: the pose model and, for PM = 1, the pair's slot of the Euler rows (ndt_newton.hpp).
template <bool SC1, bool STATE_FIRST, int PM = 0>
__device__ __forceinline__ int update_block(const PairState* Sg, PairState& S, double (*sm)[NACC], volatile double* sol, const double* __restrict__ rows, int n_src,
                                            const int pts_per_chunk, const bool chunk_rows, mi355ndt_result* res, unsigned long long* hits_total,
                                            const double step_max, const double eps, const int max_iterations, const int reduce_only, const int mt, Timeline* tl,
                                            float* pose_rows = nullptr, double* pose_rows64 = nullptr, const int ground = 0 /* MI355NDT_OPT_GROUND_CLASS */) {
  state_to_lds<SC1>(S, Sg, threadIdx.x, UPD_THREADS);
  if (threadIdx.x == 0) sol[6] = 0.0;
  if (STATE_FIRST) {
    __syncthreads();
    if (S.phase == PH_DONE) return UPD_EXIT;                                     // (block-uniform)
    if (mt == 2 && S.phase != PH_HESS) return UPD_EXIT;                          // only pairs whose Hessian pass just ran
    n_src = S.n_src;
  }
  const int lane = threadIdx.x & 63;
  const int nchunks = (n_src + pts_per_chunk - 1) / pts_per_chunk;
  const double v = reduce_pair_rows<SC1>(rows, nchunks, sums_live(lane, mt == 2, false), sm, chunk_rows);   // the Hessian pass fills H only
  if (threadIdx.x < 64) store_sums(S, lane, v, mt == 2, false, hits_total, ground);
  __syncthreads();                                                               // lane 0 reads what lanes 0..43 just stored
  if (tl) tl->stamp(9);
  if (threadIdx.x >= 128) return UPD_EXIT;
  if (threadIdx.x >= 64) {                                                       // the solve, next to wave 0
    if (mt == 0 && !reduce_only) newton_solve_side(S, sol);
    if (tl) { tl->stamp(13); tl->flush(13, 14); }
    return UPD_EXIT;
  }
  if (reduce_only) return NEWTON_DONE;
  // (latency mode: the re-basing of p for this step was computed under the sweep, by its extra workgroup -- ndt_sweep.hpp; the tag says so)
  const bool rebased = mt == 0 && S.phase == PH_STEP && S.reb_tag == (long long)S.sweeps;
  return newton_update<PM>(S, res, step_max, eps, max_iterations, mt, mt == 0 ? sol : nullptr, PM == 0 && rebased, false, pose_rows, pose_rows64, ground);
}

// One block per pair.  `rows_per_pair` = stored rows per pair (the row stride).
NDT_KERNEL void __launch_bounds__(UPD_THREADS, 2)
k_update(PairState* st, const double* __restrict__ partials, int rows_per_pair, int pts_per_chunk, int chunk_rows, mi355ndt_result* results,
         int* active_counter, int* active_list, SweepCtl* ctl, unsigned long long* hits_total,
         double step_max, double eps, int max_iterations, int reduce_only, int mt, float* euler_rows /* non-null: MI355NDT_OPT_POSE_MODEL 1 */,
         double* pcl_rows /* non-null (with euler_rows): MI355NDT_OPT_NDT_CLASS 1 */,
         int ground /* MI355NDT_OPT_GROUND_CLASS: non-zero = the sums doubled and masked, the convergence rule of ndt_ground_impl.hpp:173 (pose model 0 alone) */) {
  __shared__ double sm[UPD_WAVES][NACC];
  __shared__ double sol[SOL_WORDS];
  __shared__ PairState S;
  const int b = blockIdx.x;
  const int rc = euler_rows
      ? update_block<false, true, 1>(&st[b], S, sm, sol, partials + (size_t)b * rows_per_pair * NACC, 0, pts_per_chunk, chunk_rows != 0, &results[b], hits_total,
                                     step_max, eps, max_iterations, reduce_only, mt, nullptr, euler_rows + (size_t)b * EULER_ROW_WORDS,
                                     pcl_rows ? pcl_rows + (size_t)b * EULER_ROW_WORDS : nullptr)
      : update_block<false, true>(&st[b], S, sm, sol, partials + (size_t)b * rows_per_pair * NACC, 0, pts_per_chunk, chunk_rows != 0, &results[b], hits_total,
                                  step_max, eps, max_iterations, reduce_only, mt, nullptr, nullptr, nullptr, ground);
  if (rc == UPD_EXIT) return;
  if (threadIdx.x == 0 && rc == NEWTON_SWEEP) {
    atomicAdd(active_counter, 1);
    active_list[atomicAdd(&ctl->n_active, 1)] = b;                               // this pair takes part in the next sweep
  }
  wave_lds_sync();
  state_from_lds<false>(&st[b], S, threadIdx.x, 64);                             // the state goes back
}
