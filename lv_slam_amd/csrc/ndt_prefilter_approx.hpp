// ndt_prefilter_approx.hpp -- downsample_method = APPROX_VOXELGRID (pcl::ApproximateVoxelGrid, PCL 1.8.1 approximate_voxel_grid.hpp) over the K
// raw clouds of a batch-prefilter group, beside the VoxelGrid chain of ndt_prefilter_batch.hpp and in its conventions.
//
// PCL walks the points in input order through a history table of 512 entries {cell, count, f32 sum}: a point whose bucket
// (ix * 7171 + iy * 3079 + iz * 4231) & 511 holds another cell flushes that entry (sum / (float)count goes to the output) and starts it anew;
// after the last point the non-empty entries are flushed in table order.  What an entry gathers between two flushes is a RUN: consecutive
// points of one bucket, in input order, that share a cell.  So
//   keys    the bucket of every kept point (512: not binned -- dropped by the gate, past the cloud, or the cloud is not down-sampled);
//   sort    ONE stable 10-bit pass of the segment sort: bucket-major, input order inside a bucket;
//   heads   a sorted position opens a run when its bucket or its cell differs from its predecessor's (the cells are recomputed from the points
//           through the sorted ids; one byte per position remembers the outcome).  A run that is not the last of its bucket
//           was flushed by the point that opens the next one -- the TRIGGER --, and PCL's output order of those runs is the input order of
//           their triggers; the last run of every bucket follows, in bucket order;
//   scan    one exclusive scan per cloud over [rq trigger flags in input order][512 "bucket is not empty" flags]: a flushed run's rank is the
//           scan at its trigger's point id, a last run's is the scan at rq + bucket, and the total is the cloud's filtered count;
//   emit    the head of every run walks it -- a serial f32 chain in input order, as the table's -- and writes the centroid at its rank.
// A cloud's segment is rp = rq + 512 positions (rq: the group's raw pitch): every per-point array keeps the one pitch, the sort's padding
// positions carry key 512, and flag / pos have room for the bucket words behind the point words.
// A cloud some kept point of which has |floor(coord * inv_leaf)| >= 2^31 (PCL's cast to int is undefined there) is not down-sampled: status 2,
// the VoxelGrid route's rule and word -- its kept points go out in input order through the same scan and emit.
#pragma once
#include "ndt_prefilter_batch.hpp"

#define PFA_BUCKETS 512

// the cell of a point: ix = (int)floor(x * inv_leaf), the product f32 (status 0 only: every index fits an int)
struct PfaCell { int x, y, z; };
__device__ __forceinline__ PfaCell pfa_cell(float x, float y, float z, float inv_leaf) {
  return PfaCell{(int)floorf(x * inv_leaf), (int)floorf(y * inv_leaf), (int)floorf(z * inv_leaf)};
}
__device__ __forceinline__ PfaCell pfa_cell_of(const float* __restrict__ X, size_t pitch, float inv_leaf, size_t pi) {
  return pfa_cell(X[pi], X[pitch + pi], X[2 * pitch + pi], inv_leaf);
}
__device__ __forceinline__ bool pfa_same(const PfaCell& a, const PfaCell& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// its history-table entry: only the low 9 bits of the sum are used, so the products wrap harmlessly (unsigned arithmetic)
__device__ __forceinline__ unsigned pfa_bucket(const PfaCell& c) {
  return ((unsigned)c.x * 7171u + (unsigned)c.y * 3079u + (unsigned)c.z * 4231u) & (PFA_BUCKETS - 1u);
}

// the "grid" of one cloud from its six extremes: inv_leaf and the status (0 ok, 1 no kept point, 2 some cell index does not fit an int).
// x -> floor(x * inv_leaf) is monotone, so the extremes decide for every kept point; !(|f| < 2^31) also catches the NaN / inf products of
// an inv_leaf that overflowed.
__device__ __forceinline__ PfGrid pfa_make_grid(const int* __restrict__ mm, float leaf) {
  PfGrid g;
  memset(&g, 0, sizeof g);
  g.inv_leaf = 1.0f / leaf;
  if (mm[0] == INT_MAX) { g.status = 1; return g; }
  for (int a = 0; a < 6; a++)
    if (!(fabsf(floorf(ord2f(mm[a]) * g.inv_leaf)) < 2147483648.0f)) g.status = 2;
  return g;
}
__global__ void __launch_bounds__(64) k_pfa_grid(const int* __restrict__ mm, float leaf, PfGrid* grid, const PfbItem* __restrict__ items, int K, int* res) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= K) return;
  const PfGrid g = pfa_make_grid(mm + 6 * b, leaf);
  grid[b] = g;
  if (g.status == 2) atomicMin(&res[K + 1], items[b].id);
}

// the bucket key of position i
__device__ __forceinline__ unsigned pfa_key(const float* __restrict__ X, size_t pitch, int n, const unsigned char* __restrict__ keep, const PfGrid& g, size_t i) {
  if (i < (size_t)n && keep[i] && g.status == 0) return pfa_bucket(pfa_cell_of(X, pitch, g.inv_leaf, i));
  return PFA_BUCKETS;
}
// Keys of every position of every cloud; the 512 bucket words behind the point words of `flag` start at zero (k_pfa_heads raises them).
__global__ void __launch_bounds__(256) k_pfa_keys(const float* __restrict__ X, size_t rp, const PfbItem* __restrict__ items, int K, int nx,
                                                  const unsigned char* __restrict__ keep, const PfGrid* __restrict__ grid, unsigned* keys, int* flag) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const PfGrid g = grid[b];
  const int n = items[b].n;
  const float* Xb = X + (size_t)b * 3 * rp;
  const unsigned char* kp = keep + (size_t)b * rp;
  unsigned* kb = keys + (size_t)b * rp;
  int* fb = flag + (size_t)b * rp;
  const size_t rq = rp - PFA_BUCKETS;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) {
    kb[i] = pfa_key(Xb, rp, n, kp, g, i);
    if (i >= rq) fb[i] = 0;
  }
}

// Heads, as the flags the scan runs over.  The sorted point ids are a permutation of the segment's positions: the thread of sorted position i
// writes the point word of ITS point (1: the point is a trigger), so every point word is written once and nothing has to be cleared; the first
// position of a bucket raises the bucket's word.  Whether position i opens a run goes to heads[i] for the emit -- `heads` is the cloud's keep
// array, which a down-sampled cloud needs no more once its keys are made.  A position gathers its own point only: its predecessor's cell
// comes from the lane below (consecutive lanes hold consecutive positions, and a segment is whole waves), lane 0 gathers it.
// A cloud that is not down-sampled: its kept points, in input order, and its keep array stays what it is.
__global__ void __launch_bounds__(256) k_pfa_heads(const float* __restrict__ X, size_t rp, const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                   unsigned char* keep, const PfbItem* __restrict__ items, int K, int nx,
                                                   const PfGrid* __restrict__ grid, int* flag) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const PfGrid g = grid[b];
  const int n = items[b].n;
  const float* Xb = X + (size_t)b * 3 * rp;
  const unsigned* kb = keys + (size_t)b * rp;
  const unsigned* vb = vals + (size_t)b * rp;
  unsigned char* kp = keep + (size_t)b * rp;
  int* fb = flag + (size_t)b * rp;
  const size_t rq = rp - PFA_BUCKETS;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);         // (rp and the tile are multiples of 64: every wave is in or out as a whole)
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) {
    if (g.status != 0) { if (i < rq) fb[i] = pf_is_head(kb, kp, n, 0, i); continue; }
    const unsigned k = kb[i], v = vb[i], pk = i > 0 ? kb[i - 1] : (unsigned)PFA_BUCKETS;
    const bool binned = k != PFA_BUCKETS, follows = binned && pk == k;   // follows: not the first position of its bucket
    PfaCell c = PfaCell{0, 0, 0};
    if (binned) c = pfa_cell_of(Xb, rp, g.inv_leaf, v);
    PfaCell pc = PfaCell{__shfl_up(c.x, 1), __shfl_up(c.y, 1), __shfl_up(c.z, 1)};
    if ((threadIdx.x & 63) == 0 && follows) pc = pfa_cell_of(Xb, rp, g.inv_leaf, vb[i - 1]);
    const int trig = follows && !pfa_same(pc, c);
    if (binned && !follows) fb[rq + k] = 1;
    if (v < rq) fb[v] = trig;
    kp[i] = (binned && !follows) || trig;
  }
}

// Emit: the head of every run sums it in sorted order -- input order inside the bucket -- up to the next head or the end of the bucket, divides by
// (float)count and writes at its rank; nothing is written at or past the slot's pitch (such a cloud has raised the overflow word).
// INTENSITY: the history entry's fourth sum (downsample_all_data_: the entry's VectorXf holds x, y, z and intensity) -- from zero, in the same
// order, divided at the same flush -- from XI, the cloud's row of the intensity plane, into oi.
template <bool INTENSITY>
__device__ __forceinline__ void pfa_emit_run(const float* __restrict__ X, size_t pitch, const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                             const unsigned char* __restrict__ heads, const int* __restrict__ pos, size_t i, const PfbItem& it,
                                             const float* __restrict__ XI, float* oi) {
  if (!heads[i]) return;
  const unsigned k = keys[i];
  float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
  int cnt = 0;
  size_t j = i;
  do {                                                                // centroid += p (f32), input order
    const unsigned pi = vals[j];
    sx += X[pi]; sy += X[pitch + pi]; sz += X[2 * pitch + pi];
    if constexpr (INTENSITY) si += XI[pi];
    cnt++;
    j++;
  } while (j < pitch && keys[j] == k && !heads[j]);
  const float fn = (float)cnt;
  sx /= fn; sy /= fn; sz /= fn;                                       // centroid / (float)count
  if constexpr (INTENSITY) si /= fn;
  const bool flushed = j < pitch && keys[j] == k;                     // by the point that opens the bucket's next run
  const size_t o = (size_t)pos[flushed ? (size_t)vals[j] : pitch - PFA_BUCKETS + k];
  if (o < it.out_pitch) {
    it.out[o] = sx; it.out[it.out_pitch + o] = sy; it.out[2 * it.out_pitch + o] = sz;
    if constexpr (INTENSITY) oi[o] = si;
  }
}
template <bool INTENSITY>
__global__ void __launch_bounds__(256) k_pfa_emit(const float* __restrict__ X, size_t rp, const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                  const unsigned char* __restrict__ keep, const int* __restrict__ flag, const int* __restrict__ pos,
                                                  const PfGrid* __restrict__ grid, const PfbItem* __restrict__ items, int K, int nx, const PfbInt pi) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const PfGrid g = grid[b];
  const PfbItem it = items[b];
  const float* Xb = X + (size_t)b * 3 * rp;
  const unsigned* kb = keys + (size_t)b * rp;
  const unsigned* vb = vals + (size_t)b * rp;
  const unsigned char* kp = keep + (size_t)b * rp;
  const int* fb = flag + (size_t)b * rp;
  const int* pb = pos + (size_t)b * rp;
  const float* Ib = nullptr;
  float* oi = nullptr;
  if constexpr (INTENSITY) { Ib = pi.in + (size_t)b * rp; oi = pi.out[b]; }
  const size_t rq = rp - PFA_BUCKETS;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) {
    if (g.status == 0) { pfa_emit_run<INTENSITY>(Xb, rp, kb, vb, kp, pb, i, it, Ib, oi); continue; }
    if (i >= rq || !fb[i]) continue;
    const size_t o = (size_t)pb[i];
    if (o < it.out_pitch) {
      it.out[o] = Xb[i]; it.out[it.out_pitch + o] = Xb[rp + i]; it.out[2 * it.out_pitch + o] = Xb[2 * rp + i];
      if constexpr (INTENSITY) oi[o] = Ib[i];
    }
  }
}
