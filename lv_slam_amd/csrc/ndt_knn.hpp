// ndt_knn.hpp -- exact k-nearest and radius search over resident keyframes (mi355ndt_keyframe_knn / _knn_ids / _radius_search): what a host
// does with pcl::KdTreeFLANN::nearestKSearch / radiusSearch on a downloaded keyframe, over the keyframe's one cloud index (ndt_kffitness.hpp)
// with the keyframe left where it is.  The rules are the engine's own, stated once each elsewhere and used as they are:
//   the query      a point, moved by a column-major f32 pose as fit_query moves it -- ((T0 x + T1 y) + T2 z) + T3 -- and live iff it is finite
//                  before and after the move (icp_step_body's rule)
//   the distance   fit_d2
//   the order      ascending (d2, id), a tie to the lower point id (OlList<_, true>::before, gc_nearer); FLANN's order among equals is not emulated
//   k-NN           the k first points in that order, kept iff (double)d2 <= max_range^2 (ICP's inclusive rule; the ring walk's bound is the
//                  f32 just above the limit, as icp_make_step forms it)
//   radius         within iff d2 < r2 = (float)(radius * radius), strict (ndt_host_outlier.hpp); the count takes in EVERY point within, the
//                  list the max_nn nearest of them: the walk covers the radius whether or not the list is full (fit_rings is handed the
//                  constant bound, not list.worst)
//   unused slots   id -1, d2 +inf
// One body, knn_block: one wave per workgroup, the lane's list in LDS as OlList lays it out ([slot][lane], 2 * CAP * 64 * 4 bytes a workgroup,
// no per-lane array), CAP in {8, 32, 64} so that k = 5 does not take a CU's LDS as k = 64 does.  The launch is k_kf_fitness's flat grid over
// (item, 64-query block) entries (fit_item_table): an item = (searched keyframe, query rows, pose), its blocks on the workgroups of one XCD.
// A lattice variant and an exhaustive one (fit_tiles) are both launched and the searched keyframe's status picks the one that works.
//
// Query order.  Queries from outside do not come in cell order, so a wave's lanes may walk unrelated rings.  The cell-ordered route
// (k_knn_keys, then the engine's stable radix sort, one segment per item) materialises the moved queries as SoA rows, keys each by its
// cell in the searched keyframe's lattice (outside the lattice, not finite, no lattice: the not-binned key), and the lists run over the
// sorted positions and scatter their results by query id.  In input order a workgroup's 64 * k result words are one contiguous run of
// the output: they are written from LDS as that run, after each list has been sorted in place (OlList::ascending).
#pragma once
#include "ndt_types.hpp"
#include "ndt_fitness.hpp"
#include "ndt_kffitness.hpp"
#include "ndt_outlier.hpp"

#define KNN_MODE_KNN    0
#define KNN_MODE_RADIUS 1

// One item of a call.  q: the query rows as given ([3][qpitch], nq of them: a keyframe's, or the staged host queries); mq / order: the
// cell-ordered route's moved rows ([3][mpitch], by query id) and query ids by sorted position, both null in input order.
// tgt: the searched keyframe's index (empty: it has no point and no index).  ids / d2 / counts: the item's slices of the call's results.
struct KnnItem {
  const float* q; float* mq; const unsigned* order;
  int* ids; float* d2; int* counts;
  KfiView tgt;
  float T[16];
  unsigned qpitch, mpitch, poff; int nq, empty;    // poff: the item's first position in the sort's keys and values
};
// ... and what every item of the call shares: K = k or max_nn; bound = the walk's limit (k-NN: the f32 just above thr2; radius: r2)
struct KnnCall { double thr2; float bound; int mode, K; };

// query i of an item's given rows, moved; false when there is none or it is not finite before or after the move
__device__ __forceinline__ bool knn_query(const KnnItem& e, unsigned i, float (&q)[3]) {
  q[0] = q[1] = q[2] = 0.f;
  if (i >= (unsigned)e.nq) return false;
  const float x = e.q[i], y = e.q[e.qpitch + i], z = e.q[2 * (size_t)e.qpitch + i];
  return finite3(x, y, z) && fit_query(e.q, e.qpitch, e.nq, (int)i, e.T, q);
}

// The cell-ordered route's first stage, grid.y = the item: the moved query (NaN where there is none or it is not live) into the item's
// rows, its cell in the searched keyframe's lattice as the sort's key, its position as the sort's value.
__global__ void __launch_bounds__(256) k_knn_keys(const KnnItem* __restrict__ items, unsigned* keys, unsigned* vals) {
  const KnnItem e = items[blockIdx.y];
  const unsigned pitch = ((unsigned)e.nq + 63u) & ~63u;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= pitch || !e.mq) return;
  float q[3];
  const bool live = knn_query(e, i, q);
  const float nan = __int_as_float(0x7fc00000);
  float* M = e.mq;
  M[i] = live ? q[0] : nan; M[e.mpitch + i] = live ? q[1] : nan; M[2 * (size_t)e.mpitch + i] = live ? q[2] : nan;
  unsigned key = (1u << KFI_CELL_BITS) - 1u;
  if (live && !e.empty) {
    const GridDesc& g = *e.tgt.gd;
    if (g.status == GRID_OK) {
      const float c0 = floorf(q[0] * g.inv_leaf) - (float)g.min_b[0];
      const float c1 = floorf(q[1] * g.inv_leaf) - (float)g.min_b[1];
      const float c2 = floorf(q[2] * g.inv_leaf) - (float)g.min_b[2];
      if (c0 >= 0.f && c0 < (float)g.div_b[0] && c1 >= 0.f && c1 < (float)g.div_b[1] && c2 >= 0.f && c2 < (float)g.div_b[2])
        key = (unsigned)((int)c0 + (int)c1 * g.mul1 + (int)c2 * g.mul2);
    }
  }
  keys[e.poff + i] = key;
  vals[e.poff + i] = i;
}

// One block of 64 queries of one item.  LATTICE: the searched keyframe has a lattice (the ring walk); else it has none (GRID_CAP: the
// exhaustive walk, every lane calls) or nothing to search (every count 0).  The WHOLE workgroup runs to the end: the exits are uniform.
template <int CAP, bool LATTICE>
__device__ __forceinline__ void knn_block(const KnnItem& e, const KnnCall& c, int bx) {
  __shared__ float lst[CAP][OL_LANES];
  __shared__ unsigned lid[CAP][OL_LANES];
  const int status = e.empty ? GRID_EMPTY : e.tgt.gd->status;
  if (LATTICE != (status == GRID_OK)) return;
  const int lane = threadIdx.x, K = c.K;
  const unsigned p = (unsigned)bx * OL_LANES + (unsigned)lane;
  // the lane's query: position p of the given rows, or of the sorted order
  unsigned qid = p;
  float q[3] = {0.f, 0.f, 0.f};
  bool live = false;
  if (e.order) {
    qid = p < (unsigned)e.nq ? e.order[p] : 0xFFFFFFFFu;
    if (qid < (unsigned)e.nq) {
      q[0] = e.mq[qid]; q[1] = e.mq[e.mpitch + qid]; q[2] = e.mq[2 * (size_t)e.mpitch + qid];
      live = finite3(q[0], q[1], q[2]);
    }
  } else {
    live = knn_query(e, p, q);
  }
  OlList<CAP, true> list;
  list.init(lst, K, lid);
  int within = 0;
  const float bound = c.bound;
  const bool radius = c.mode == KNN_MODE_RADIUS;
  const double thr2 = c.thr2;
  float walk_best = radius ? bound : list.worst;   // what fit_rings reads to stop: the radius, or the list's worst entry once it is full
  auto take = [&](float d2, unsigned id) {
    if (radius) { if (d2 < bound) { within++; list.insert(d2, id); } }
    else if ((double)d2 <= thr2) { list.insert(d2, id); walk_best = list.worst; }
  };
  if constexpr (LATTICE) {
    if (live) {
      const float* X = e.tgt.sorted;
      const unsigned* ids = e.tgt.ids;
      const size_t tp = e.tgt.pitch;
      fit_rings(q, *e.tgt.gd, e.tgt.words, e.tgt.runs, 1 << 30, bound, walk_best, [&](unsigned j0, unsigned j1) {
        for (unsigned t = j0; t < j1; t++) take(fit_d2(q, X[t], X[tp + t], X[2 * tp + t]), ids[t]);
      });
    }
  } else {
    fit_tiles<OL_LANES>(e.tgt.rows, e.tgt.pitch, status == GRID_CAP ? e.tgt.n : 0, [&](float x, float y, float z, unsigned t) {
      if (live) take(fit_d2(q, x, y, z), t);
    });
  }
  const int count = radius ? within : list.cnt;
  // unused slots, then the list in place in ascending (d2, id): a real entry at +inf comes before the unused ones
  for (int s = list.cnt; s < K; s++) { lst[s][lane] = __int_as_float(0x7f800000); lid[s][lane] = 0xFFFFFFFFu; }
  {
    int m = 0;
    list.ascending([&](float v, unsigned vi) { lst[m][lane] = v; lid[m][lane] = vi; m++; });
  }
  if (e.order) {                                  // by query id: K words of this lane's own column
    if (qid < (unsigned)e.nq) {
      for (int s = 0; s < K; s++) { e.ids[(size_t)qid * K + s] = (int)lid[s][lane]; e.d2[(size_t)qid * K + s] = lst[s][lane]; }
      e.counts[qid] = count;
    }
    return;
  }
  __syncthreads();                                // the run below reads the other lanes' columns
  const size_t base = (size_t)bx * OL_LANES;
  const int rows = e.nq - (int)base < OL_LANES ? e.nq - (int)base : OL_LANES;
  for (int w = lane; w < rows * K; w += OL_LANES) {
    const int l = w / K, s = w - l * K;
    e.ids[base * K + w] = (int)lid[s][l];
    e.d2[base * K + w] = lst[s][l];
  }
  if (lane < rows) e.counts[base + lane] = count;
}

template <int CAP, bool LATTICE>
__global__ void __launch_bounds__(OL_LANES) k_kf_knn(const FitItem* __restrict__ items, const int* __restrict__ gstart, const KnnItem* __restrict__ tab,
                                                     KnnCall c) {
  FitItem it;
  int bx;
  if (!fit_item(items, gstart, it, bx)) return;
  const KnnItem e = tab[it.pair];
  knn_block<CAP, LATTICE>(e, c, bx);
}
