// ndt_outlier_batch.hpp -- the outlier removal of ndt_outlier.hpp over the clouds K batch slots hold (mi355ndt_batch_remove_outliers): every
// stage is one launch for all K clouds of a group, the statistics are formed on the device, and the group waits for the device once.
//
// A group's clouds are staged from their slots into the scratch as [cloud][3][rp] (rp: the group's largest count rounded to 64, not the slot
// pitch -- mi355ndt_sequence_run_raw reserves slots for raw counts, several times the filtered ones); keys, ids, flag, pos and dist are
// [cloud][rp].  The K cloud indexes are pools in the scratch for the duration of the group: KfiHead heads[K], a GridDesc per cloud for the
// kernels that index gd[b] (the segmented sort's key pass, k_fit_mark / k_fit_rank / k_fit_runs: all used as they are, a cloud = a "target"),
// BitWord words[K][nwc], runs[K][rp + 1], sorted[K][3][rp], ids[K][rp].  The cell rule is k_kfi_grid's per cloud (kfi_cell_rule), with the
// cell cap the one-cloud surface would give the cloud, so a cloud has a lattice here iff it has one there.
//
// The k-NN launch is flat over (cloud, 64-query block) items dealt by fit_item_table -- a cloud's blocks on the workgroups of one XCD, as
// k_kf_fitness has them -- with ol_knn's body: one wave per workgroup, the lists in LDS [slot][lane].  Clouds of 1 point and of 100,000 share
// the launch; the clouds without a lattice are served by the exhaustive variant in a launch of its own over the same table.
//
// StatisticalOutlierRemoval's statistics are two dependent f64 chains over all n values of a cloud in index order: one wave per chain, K
// clouds side by side (k_olb_stats).  The compaction reads the staged copy and writes the slot rows, so no survivor can land on a row that
// has not been read yet, whatever order the workgroups run in.
#pragma once
#include "ndt_outlier.hpp"
#include "ndt_prefilter_batch.hpp"

// result words of a group of K clouds: [0, K) surviving counts and [K], [K + 1] as k_pfb_scan_offsets leaves them (PFB_RES_WORDS; a
// surviving count never exceeds its slot), then per cloud the lattice's status and the searchable points
#define OLB_RES_WORDS(K) (PFB_RES_WORDS(K) + 2 * (size_t)(K))
#define OLB_STAT_AT(K)   PFB_RES_WORDS(K)
// doubles per cloud of the statistics' result: mean, stddev, threshold
#define OLB_STAT_DOUBLES 3

// one cloud of the k-NN launch: its index, its row of dist[] and of keep[]
struct OlbCloud { KfiView v; float* dist; int* keep; };

__global__ void __launch_bounds__(256) k_olb_begin(unsigned* mm, int* res, int* cnt, const PfbItem* __restrict__ items, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * K) mm[i] = 0u;                      // (k_minmax's "no finite point yet")
  if (i < (int)OLB_RES_WORDS(K)) res[i] = (i == K || i == K + 1) ? INT_MAX : 0;
  if (i < K) cnt[i] = items[i].n;
}

// Stage: the slot's points into the cloud's segment, zeros behind them to the segment's pitch.  INTENSITY: the intensity row of a slot that
// carries one (pi.out[b], the row the emit compacts into) goes into the cloud's row of the plane beside the segments (pi.in).
template <bool INTENSITY>
__global__ void __launch_bounds__(256) k_olb_stage(const PfbItem* __restrict__ items, int K, int nx, float* X, size_t rp, const PfbInt pi) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const PfbItem it = items[b];
  float* Xb = X + (size_t)b * 3 * rp;
  const float* si = nullptr;
  if constexpr (INTENSITY) si = pi.out[b];
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) {
    const bool in = i < (size_t)it.n;
    Xb[i] = in ? it.out[i] : 0.f;
    Xb[rp + i] = in ? it.out[it.out_pitch + i] : 0.f;
    Xb[2 * rp + i] = in ? it.out[2 * it.out_pitch + i] : 0.f;
    if constexpr (INTENSITY) if (si) pi.in[(size_t)b * rp + i] = in ? si[i] : 0.f;
  }
}

// Grid: k_kfi_grid's rule per cloud; max_cells as kfi_layout gives a cloud of this size on the one-cloud surface.  The pools' descriptor
// carries the cloud's place in the word pool (k_fit_mark / k_fit_rank / k_fit_runs), the header is what the k-NN reads.
__global__ void __launch_bounds__(64) k_olb_grid(const unsigned* __restrict__ mm, float cell0, const PfbItem* __restrict__ items, int K, unsigned nwc,
                                                 GridDesc* gds, KfiHead* heads, int* stat) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= K) return;
  const size_t pitch = ((size_t)items[b].n + 63) & ~(size_t)63;
  const size_t cap = 64 * pitch < 4096 ? 4096 : 64 * pitch;
  GridDesc g = kfi_cell_rule(mm + 6 * b, cell0, (int)(cap < (size_t)KFI_MAX_CELLS ? cap : (size_t)KFI_MAX_CELLS));
  g.word_off = (unsigned)b * nwc;
  gds[b] = g;
  heads[b].gd = g;
  heads[b].n_fin = 0;
  stat[2 * b] = g.status;
  stat[2 * b + 1] = 0;
}

// Gather: k_kfi_gather per cloud -- the points and their ids in cell order, the searchable points counted into the header and the host's word
__global__ void __launch_bounds__(256) k_olb_gather(const float* __restrict__ X, size_t rp, const int* __restrict__ cnt, const unsigned* __restrict__ vals,
                                                    float* __restrict__ sorted, unsigned* __restrict__ ids, KfiHead* heads, int* stat, int K, int nx) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const int n = cnt[b];
  const float* Xb = X + (size_t)b * 3 * rp;
  const unsigned* vb = vals + (size_t)b * rp;
  float* sb = sorted + (size_t)b * 3 * rp;
  unsigned* ib = ids + (size_t)b * rp;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  int c = 0;
  for (size_t i0 = (size_t)bx * RS_TILE; i0 < end; i0 += 256) {   // (a uniform loop: the count is a block-wide vote)
    const size_t i = i0 + threadIdx.x;
    bool fin = false;
    if (i < end) {
      const unsigned v = vb[i];
      const float x = Xb[v], y = Xb[rp + v], z = Xb[2 * rp + v];
      ib[i] = v;
      sb[i] = x; sb[rp + i] = y; sb[2 * rp + i] = z;
      fin = v < (unsigned)n && finite3(x, y, z);
    }
    c += __syncthreads_count(fin);
  }
  if (threadIdx.x == 0 && c) { atomicAdd(&heads[b].n_fin, c); atomicAdd(stat + 2 * b + 1, c); }
}

// RADIUS with min_neighbors = 0: every searchable point is kept (no search, no index)
__global__ void __launch_bounds__(256) k_olb_finite(const float* __restrict__ X, size_t rp, const PfbItem* __restrict__ items, int K, int nx, int* keep) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const size_t n = (size_t)items[b].n;
  const float* Xb = X + (size_t)b * 3 * rp;
  int* kb = keep + (size_t)b * rp;
  const size_t end = std::min(std::min(rp, n), (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) kb[i] = finite3(Xb[i], Xb[rp + i], Xb[2 * rp + i]) ? 1 : 0;
}

// The k-NN of every cloud of the group: the flat grid of k_kf_fitness over (cloud, block of OL_LANES queries) items, ol_knn's body per block.
// LATTICE picks the clouds with a lattice, the other instantiation those without (GRID_CAP); ol_knn decides by the cloud's status.
template <int CAP, bool LATTICE>
__global__ void __launch_bounds__(OL_LANES) k_olb_knn(const FitItem* __restrict__ items, const int* __restrict__ gstart, const OlbCloud* __restrict__ clouds,
                                                      int method, int K, float r2) {
  FitItem it;
  int bx;
  if (!fit_item(items, gstart, it, bx)) return;
  const OlbCloud c = clouds[it.pair];
  ol_knn<CAP, LATTICE>(c.v, (unsigned)bx, method, K, r2, c.dist, c.keep);
}

// Statistics: one workgroup of two waves per cloud, one dependent f64 chain each -- wave 0: sum += d, wave 1: sq += d * d -- strictly in
// index order over all n values of dist[] (the zeros of the non-valid points included).  Every step the lanes load 64 values, coalesced, and
// each lane widens its own (wave 1: and squares it, one rounding, as the chain would); then every lane of the wave runs the same 64 adds on
// the terms broadcast lane by lane (two v_readlane_b32 and one v_add_f64 per value: the vector unit issues little but the chain's own adds,
// and the wave does not diverge).  The next step's load is in flight under them.  Then, each a separately rounded operation:
// mean = sum / nv, var = (sq - sum * sum / nv) / (nv - 1), stddev = sqrt(var), threshold = mean + mul * stddev; nv = n_fin when
// n_fin >= mean_k + 1, else 0 (a NaN threshold, which removes nothing).
#define OLB_STATS_THREADS 128
__global__ void __launch_bounds__(OLB_STATS_THREADS) k_olb_stats(const float* __restrict__ dist, size_t rp, const PfbItem* __restrict__ items,
                                                                 const int* __restrict__ stat, int mean_k, double mul, double* out) {
  __shared__ double sq_of_wave1;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = items[b].n;
  const float* D = dist + (size_t)b * rp;
  double acc = 0.0;
  float cur = lane < n ? D[lane] : 0.f;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int nxt = i0 + 64 + lane;
    const float ahead = nxt < n ? D[nxt] : 0.f;
    const double d = (double)cur;
    const double term = wave ? d * d : d;
    const int lo = __double2loint(term), hi = __double2hiint(term);
    const int m = n - i0;
    if (m >= 64) {
#pragma unroll
      for (int t = 0; t < 64; t++) acc += __hiloint2double(__builtin_amdgcn_readlane(hi, t), __builtin_amdgcn_readlane(lo, t));
    } else {
      for (int t = 0; t < m; t++) acc += __shfl(term, t);
    }
    cur = ahead;
  }
  if (wave == 1 && lane == 0) sq_of_wave1 = acc;
  __syncthreads();
  if (wave != 0) return;
  const double sum = acc, sq = sq_of_wave1;
  const int nf = stat[2 * b + 1];
  const double nv = nf >= mean_k + 1 ? (double)nf : 0.0;
  const double mean = sum / nv;
  const double var = (sq - sum * sum / nv) / (nv - 1.0);
  const double stddev = sqrt(var);
  if (lane == 0) {
    out[OLB_STAT_DOUBLES * b] = mean;
    out[OLB_STAT_DOUBLES * b + 1] = stddev;
    out[OLB_STAT_DOUBLES * b + 2] = mean + mul * stddev;
  }
}

// STATISTICAL: removed iff (double)dist > threshold (a NaN threshold removes nothing); positions past the cloud: 0
__global__ void __launch_bounds__(256) k_olb_flag(const float* __restrict__ dist, size_t rp, const PfbItem* __restrict__ items, const double* __restrict__ st,
                                                  int K, int nx, int* flag) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const size_t n = (size_t)items[b].n;
  const double threshold = st[OLB_STAT_DOUBLES * b + 2];
  const float* D = dist + (size_t)b * rp;
  int* fb = flag + (size_t)b * rp;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) fb[i] = (i < n && !((double)D[i] > threshold)) ? 1 : 0;
}

// Emit: the survivors, in order, from the staged copy into the slot's rows; the rows between the new count (res[b], k_pfb_scan_offsets) and
// the old one are zeroed -- behind the old count they are zero already, as an upload leaves them.  Survivors land below the new count and
// zeros at or above it: no two threads write one row, and nobody reads the slot.  INTENSITY: the same for the intensity row of a slot that
// carries one, out of the staged plane.
template <bool INTENSITY>
__global__ void __launch_bounds__(256) k_olb_emit(const float* __restrict__ X, size_t rp, const int* __restrict__ flag, const int* __restrict__ pos,
                                                  const PfbItem* __restrict__ items, const int* __restrict__ res, int K, int nx, const PfbInt pi) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const PfbItem it = items[b];
  const size_t n = (size_t)it.n, m = (size_t)res[b];
  const float* Xb = X + (size_t)b * 3 * rp;
  const int* fb = flag + (size_t)b * rp;
  const int* pb = pos + (size_t)b * rp;
  const float* Ib = nullptr;
  float* oi = nullptr;
  if constexpr (INTENSITY) { Ib = pi.in + (size_t)b * rp; oi = pi.out[b]; }
  const size_t end = std::min(std::min(rp, n), (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) {
    if (fb[i]) {
      const size_t o = (size_t)pb[i];
      if (o < m) {
        it.out[o] = Xb[i]; it.out[it.out_pitch + o] = Xb[rp + i]; it.out[2 * it.out_pitch + o] = Xb[2 * rp + i];
        if constexpr (INTENSITY) if (oi) oi[o] = Ib[i];
      }
    }
    if (i >= m) {
      it.out[i] = 0.f; it.out[it.out_pitch + i] = 0.f; it.out[2 * it.out_pitch + i] = 0.f;
      if constexpr (INTENSITY) if (oi) oi[i] = 0.f;
    }
  }
}
