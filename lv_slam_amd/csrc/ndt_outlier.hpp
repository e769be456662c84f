// ndt_outlier.hpp -- outlier removal over the resident prefilter result (mi355ndt_prefilter_outliers): the last stage of
// PrefilteringNodelet::filter (src/lidar_odometry/prefiltering_nodelet.cpp:128, 150-161) -- pcl::StatisticalOutlierRemoval (the in-code
// default, :61-70) and pcl::RadiusOutlierRemoval (:71-78, built by the reference and never assigned: it does not run there).
//
// Both filters ask one question per point: the K smallest squared distances to the OTHER searchable points (three finite coordinates).
//   STATISTICAL  nearestKSearch(mean_k + 1) returns the point itself first (d2 = 0, the smallest there is) and the filter drops it: what is
//                left is the mean_k smallest distances to the others, K = mean_k.  dist = (float)(sum of (double)sqrtf(d2), ascending / mean_k).
//   RADIUS       kept iff at least min_neighbors others have d2 < r2 (strict): the K-th smallest distance to the others, K = min_neighbors, is < r2.
// The multiset of the K smallest does not depend on the visiting order or on how ties are broken, so the search is exact word for word.
//
// The index is a cloud index (ndt_kffitness.hpp: lattice, rank words, run starts, points and ids in cell order), this surface's own and
// rebuilt by every call.  The list of one query is filled in one place, knn_fill, which the GICP covariances share (ndt_gicp.hpp): with a
// lattice the queries are taken in cell order -- a wave's lanes sit in neighbouring cells and walk similar rings -- and the results scattered
// by point id; fit_rings drives the walk with the list's worst entry as `best` once the list is full.  A cloud without a lattice (GRID_CAP:
// a stray point at 1e12 m) is walked exhaustively (fit_tiles), the queries in input order.  Each lane's list lives in LDS, [slot][lane]: a
// wave's access to one slot touches 64 consecutive words (no bank conflict), and no lane needs scratch memory for it.  The two paths are two
// kernels here (k_ol_knn, k_ol_knn_brute): one wave per workgroup, occupancy bound by LDS, and the lattice kernel does not carry the 3 KB tile.
#pragma once
#include "ndt_types.hpp"
#include "ndt_fitness.hpp"
#include "ndt_kffitness.hpp"

#define OL_LANES 64                      // one wave per workgroup: a wave whose lanes walk far gives its LDS back on its own
#define OL_MAX_K 64
#define OL_STATISTICAL 1
#define OL_RADIUS 2

// the K smallest squared distances a lane has seen, unsorted, with the largest of them (`worst`, at `wslot`) tracked: a candidate that does
// not beat it costs one compare.  worst = +inf until the list is full -- what fit_rings reads as `best`.
// IDS: every entry carries its point id in a second column and the order is (d2, id) -- the GICP covariances (ndt_gicp.hpp), whose sums
// depend on which of two equally distant points is kept and on the order they are added in.  Without ids, equal distances are equal entries.
template <int CAP, bool IDS = false>
struct OlList {
  static constexpr bool ids = IDS;
  float* L;                              // this lane's column: slot s at L[s * OL_LANES]
  unsigned* I;                           // (IDS) the ids' column
  int K, cnt, wslot;
  float worst;
  unsigned wid;
  __device__ __forceinline__ void init(float (*lst)[OL_LANES], int k, unsigned (*ids)[OL_LANES] = nullptr) {
    L = &lst[0][threadIdx.x]; I = IDS ? &ids[0][threadIdx.x] : nullptr;
    K = k; cnt = 0; wslot = 0; worst = __int_as_float(0x7f800000); wid = 0u;
  }
  static __device__ __forceinline__ bool before(float a, unsigned ia, float b, unsigned ib) {
    if constexpr (IDS) return a < b || (a == b && ia < ib);
    else return a < b;
  }
  __device__ __forceinline__ unsigned id_at(int s) const { if constexpr (IDS) return I[s * OL_LANES]; else return 0u; }
  __device__ __forceinline__ void rescan() {
    float w = L[0];
    unsigned wi = id_at(0);
    int ws = 0;
    for (int s = 1; s < K; s++) {
      const float v = L[s * OL_LANES];
      const unsigned vi = id_at(s);
      if (before(w, wi, v, vi)) { w = v; wi = vi; ws = s; }
    }
    worst = w; wid = wi; wslot = ws;
  }
  __device__ __forceinline__ void insert(float d2, unsigned id = 0u) {
    if (cnt < K) {
      L[cnt * OL_LANES] = d2;
      if constexpr (IDS) I[cnt * OL_LANES] = id;
      if (++cnt == K) rescan();
    } else if (before(d2, id, worst, wid)) {
      L[wslot * OL_LANES] = d2;
      if constexpr (IDS) I[wslot * OL_LANES] = id;
      rescan();
    }
  }
  // the entries in ascending order, by selection (the list is consumed): take(d2, id) for each
  template <typename Take>
  __device__ __forceinline__ void ascending(Take take) {
    for (int m = 0; m < K; m++) {
      float v = L[m * OL_LANES];
      unsigned vi = id_at(m);
      int at = m;
      for (int t = m + 1; t < K; t++) {
        const float u = L[t * OL_LANES];
        const unsigned ui = id_at(t);
        if (before(u, ui, v, vi)) { v = u; vi = ui; at = t; }
      }
      L[at * OL_LANES] = L[m * OL_LANES];
      if constexpr (IDS) I[at * OL_LANES] = I[m * OL_LANES];
      take(v, vi);
    }
  }
  // STATISTICAL: s += (double)sqrtf(d2) in ascending order; (float)(s / mean_k).  sqrtf, correctly rounded under
  // the build's -fhip-fp32-correctly-rounded-divide-sqrt -- not __fsqrt_rn, which this toolchain maps to the native approximate
  // square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined (one ulp off in some terms, which reaches dist[] now and then).
  __device__ __forceinline__ float mean_distance() {
    double s = 0.0;
    ascending([&](float v, unsigned) { s += (double)sqrtf(v); });
    return (float)(s / (double)K);
  }
  __device__ __forceinline__ bool full() const { return cnt == K; }
};

// keep = 1 for each searchable point (RADIUS with min_neighbors = 0: no search, no index)
__global__ void __launch_bounds__(256) k_ol_finite(const float* __restrict__ rows, size_t pitch, int n, int* keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) keep[i] = finite3(rows[i], rows[pitch + i], rows[2 * pitch + i]) ? 1 : 0;
}

// The list of one lane's query, filled: the `list.K` nearest searchable points of the cloud, SKIP_SELF: other than the query itself.
// LATTICE: query j = the point at sorted position j (a lattice bins every searchable point: positions 0 .. n_fin - 1), the ring walk,
// nothing beyond max_range.  Otherwise: query j = point j of the rows, the exhaustive walk -- every lane of the workgroup (OL_LANES) calls.
// Returns whether the lane has a query; id = its point id.
template <bool LATTICE, bool SKIP_SELF, typename List>
__device__ __forceinline__ bool knn_fill(const KfiView& v, unsigned j, float max_range, List& list, unsigned& id) {
  const size_t pitch = v.pitch;
  float q[3] = {0.f, 0.f, 0.f};
  id = j;
  if constexpr (LATTICE) {
    if (j >= (unsigned)v.n_fin()) return false;
    const float* X = v.sorted;
    q[0] = X[j]; q[1] = X[pitch + j]; q[2] = X[2 * pitch + j];
    id = v.ids[j];
    fit_rings(q, *v.gd, v.words, v.runs, 1 << 30, max_range, list.worst, [&](unsigned j0, unsigned j1) {
      for (unsigned t = j0; t < j1; t++) {
        if (SKIP_SELF && t == j) continue;
        unsigned tid = 0u;
        if constexpr (List::ids) tid = v.ids[t];
        list.insert(fit_d2(q, X[t], X[pitch + t], X[2 * pitch + t]), tid);
      }
    });
    return true;
  } else {
    bool live = false;
    if (j < (unsigned)v.n) {
      q[0] = v.rows[j]; q[1] = v.rows[pitch + j]; q[2] = v.rows[2 * pitch + j];
      live = finite3(q[0], q[1], q[2]);
    }
    fit_tiles<OL_LANES>(v.rows, pitch, v.n, [&](float x, float y, float z, unsigned t) {
      if (live && !(SKIP_SELF && t == j)) list.insert(fit_d2(q, x, y, z), t);
    });
    return live;
  }
}

// One lane per searchable point.  method STATISTICAL: dist[id]; RADIUS: keep[id].  The caller has zeroed both; non-searchable points keep
// their zero.  Both kernels are launched and the cloud's status picks the one that works.  blk: the workgroup's block of OL_LANES queries
// within its cloud (the K-cloud launch of ndt_outlier_batch.hpp takes it from its item table).
template <int CAP, bool LATTICE>
__device__ __forceinline__ void ol_knn(const KfiView& v, unsigned blk, int method, int K, float r2, float* dist, int* keep) {
  __shared__ float lst[CAP][OL_LANES];
  if (v.gd->status != (LATTICE ? GRID_OK : GRID_CAP)) return;
  if (method == OL_STATISTICAL && v.n_fin() < K + 1) return;   // nearestKSearch(mean_k + 1) comes back short: dist = 0, not valid
  OlList<CAP> list;
  list.init(lst, K);
  unsigned id;
  if (!knn_fill<LATTICE, true>(v, blk * OL_LANES + threadIdx.x, method == OL_RADIUS ? r2 : __int_as_float(0x7f800000), list, id)) return;
  if (method == OL_STATISTICAL) dist[id] = list.mean_distance();
  else keep[id] = (list.full() && list.worst < r2) ? 1 : 0;
}
template <int CAP>
__global__ void __launch_bounds__(OL_LANES) k_ol_knn(KfiView v, int method, int K, float r2, float* dist, int* keep) { ol_knn<CAP, true>(v, blockIdx.x, method, K, r2, dist, keep); }
template <int CAP>
__global__ void __launch_bounds__(OL_LANES) k_ol_knn_brute(KfiView v, int method, int K, float r2, float* dist, int* keep) { ol_knn<CAP, false>(v, blockIdx.x, method, K, r2, dist, keep); }

// STATISTICAL: removed iff (double)dist > threshold (a NaN threshold removes nothing); positions past n: 0
__global__ void __launch_bounds__(256) k_ol_flag(const float* __restrict__ dist, int n, size_t pitch, double threshold, int* flag) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pitch) return;
  flag[i] = (i < (size_t)n && !((double)dist[i] > threshold)) ? 1 : 0;
}

// the survivors, in order, into rows of the same pitch (the caller has zeroed `out`: the tail stays zero to the pitch).  INTENSITY: the rows
// are [4][pitch] and the fourth is compacted with the same pos[].
template <bool INTENSITY>
__global__ void __launch_bounds__(256) k_ol_compact(const float* __restrict__ rows, size_t pitch, const int* __restrict__ flag,
                                                    const int* __restrict__ pos, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pitch || !flag[i]) return;
  const int o = pos[i];
  out[o] = rows[i]; out[pitch + o] = rows[pitch + i]; out[2 * pitch + o] = rows[2 * pitch + i];
  if constexpr (INTENSITY) out[3 * pitch + o] = rows[3 * pitch + i];
}
