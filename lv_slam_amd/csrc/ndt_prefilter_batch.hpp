// ndt_prefilter_batch.hpp -- the prefilter of ndt_prefilter.hpp over K raw clouds at once (mi355ndt_batch_prefilter): every stage is one launch for
// all K, the result goes straight into the clouds' batch slots.
//
// The K raw clouds of a group live in the scratch as [cloud][3][rp] (rp: the group's pitch, a multiple of 64); keep, keys, ids, flag and pos are
// [cloud][rp].  A cloud is one segment of the sort (ndt_segsort.hpp: n_segments = K, 31 key bits, three 11-bit passes), and every per-point
// kernel here gives a cloud `nx` workgroups placed by xcd_map like the sort's own: a cloud's rows, keys and ids stay in one XCD's L2 from the
// flag kernel to the emit.  Positions are size_t wherever a cloud index is multiplied in (271 clouds of 131,072 points: 35.5 M positions).
// The per-point arithmetic -- the gate, the voxel key, the head test, the centroid walk -- is ndt_prefilter.hpp's, called from both files.
// A group that carries PointXYZI's intensity has a plane I[cloud][rp] behind its rows (PfbInt): the staging fills it and the emit kernels'
// INTENSITY instantiations walk it; gate, keys, sort, heads and scans never look at it, and the [cloud][3][rp] addressing is what it was.
#pragma once
#include "ndt_prefilter.hpp"
#include "ndt_segsort.hpp"

// one raw cloud of a group: where its filtered points go (the rows of its batch slot, out_pitch floats each), its raw point count, and its
// number within the call (what the two "first cloud that ..." words hold)
struct PfbItem { float* out; unsigned long long out_pitch; int n, id; };
// the optional rigid move in front of the gate, row-major 3x4: m[4 * a + c] = T(a, c)
struct PfbMove { int on; float m[12]; };
// the fourth channel of a group, a plane of its own beside the [cloud][3][rp] rows: in = I[cloud][rp], and per cloud the row its filtered
// intensities go to -- out_pitch floats, position for position the item's rows (null: this cloud carries none).  Only the staging and the
// emit kernels look at it, and only in their INTENSITY instantiations.
struct PfbInt { float* in; float* const* out; };
// result words of a group of K clouds: [0, K) filtered counts, [K] the first cloud whose count exceeds its slot, [K + 1] the first cloud whose
// leaf is too small for its extent (INT_MAX: none)
#define PFB_RES_WORDS(K) ((size_t)(K) + 2)

__global__ void __launch_bounds__(256) k_pfb_begin(int* mm, int* res, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 6 * K) mm[i] = (i % 6) < 3 ? INT_MAX : INT_MIN;
  if (i < K + 2) res[i] = i < K ? 0 : INT_MAX;
}

// Flag: the move (pcl::transformPointCloud(in, out, Eigen::Matrix4f) of PCL 1.8.1: every product and sum a separately rounded f32 operation;
// a point with a non-finite coordinate is left as it is and fails the finite test), written back to the rows -- the centroids sum moved points --,
// then the vertical-angle calibration (pf_calibrate) under the same rule, then the gate and the cloud's extremes: cloud_callback's order.
__global__ void __launch_bounds__(256) k_pfb_flag(float* X, size_t rp, const PfbItem* __restrict__ items, int K, int nx, int use_df, double dnear,
                                                  double dfar, const PfbMove mv, const PfCal cal, unsigned char* keep, int* mm) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const int n = items[b].n;
  float* Xb = X + (size_t)b * 3 * rp;
  unsigned char* kp = keep + (size_t)b * rp;
  PfExt ext;
  for (int i = bx * 256 + (int)threadIdx.x; i < n; i += nx * 256) {
    float x = Xb[i], y = Xb[rp + i], z = Xb[2 * rp + i];
    const bool fin = finite3(x, y, z);
    if (mv.on && fin) {
      const float tx = ((mv.m[0] * x + mv.m[1] * y) + mv.m[2] * z) + mv.m[3];
      const float ty = ((mv.m[4] * x + mv.m[5] * y) + mv.m[6] * z) + mv.m[7];
      const float tz = ((mv.m[8] * x + mv.m[9] * y) + mv.m[10] * z) + mv.m[11];
      x = tx; y = ty; z = tz;
    }
    const bool turn = cal.on && finite3(x, y, z);                    // (a move may have taken the point out of f32's range)
    if (turn) pf_calibrate(x, y, z, cal.sn, cal.cs);
    if ((mv.on && fin) || turn) { Xb[i] = x; Xb[rp + i] = y; Xb[2 * rp + i] = z; }
    const bool ok = pf_gate(x, y, z, use_df, dnear, dfar);
    kp[i] = ok ? 1 : 0;
    if (ok) ext.take(x, y, z);
  }
  ext.commit(mm + 6 * b);
}

// Grid: one PfGrid per cloud, decided here; nobody waits for it.  A cloud whose leaf is too small keeps status 2: its keys are all "not binned",
// its heads are its kept points.
__global__ void __launch_bounds__(64) k_pfb_grid(const int* __restrict__ mm, float leaf, PfGrid* grid, const PfbItem* __restrict__ items, int K, int* res) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= K) return;
  const PfGrid g = pf_make_grid(mm + 6 * b, leaf);
  grid[b] = g;
  if (g.status == 2) atomicMin(&res[K + 1], items[b].id);
}

// Keys of every position of every cloud (positions past the cloud: not binned).  The point id of position i is i: the sort's first pass supplies it.
__global__ void __launch_bounds__(256) k_pfb_keys(const float* __restrict__ X, size_t rp, const PfbItem* __restrict__ items, int K, int nx,
                                                  const unsigned char* __restrict__ keep, const PfGrid* __restrict__ grid, unsigned* keys) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const PfGrid g = grid[b];
  const int n = items[b].n;
  const float* Xb = X + (size_t)b * 3 * rp;
  const unsigned char* kp = keep + (size_t)b * rp;
  unsigned* kb = keys + (size_t)b * rp;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) kb[i] = pf_cell_key(Xb, rp, n, kp, g, i);
}

// Heads: of the voxel runs of a down-sampled cloud, else the kept points (leaf <= 0 for all, or this cloud's leaf too small)
__global__ void __launch_bounds__(256) k_pfb_heads(const unsigned* __restrict__ keys, const unsigned char* __restrict__ keep, size_t rp,
                                                   const PfbItem* __restrict__ items, int K, int nx, const PfGrid* __restrict__ grid, int downsample, int* flag) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const int ds = downsample && grid[b].status == 0;
  const int n = items[b].n;
  const unsigned* kb = keys + (size_t)b * rp;
  const unsigned char* kp = keep + (size_t)b * rp;
  int* fb = flag + (size_t)b * rp;
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) fb[i] = pf_is_head(kb, kp, n, ds, i);
}

// Positions: the exclusive scan of ndt_prefilter.hpp per cloud -- emit positions restart at 0 in every cloud; tmp: `chunks` words per cloud.
// The middle kernel knows every cloud's total: the count goes to res[b], and a count that exceeds its slot raises the overflow word.
__global__ void __launch_bounds__(1024) k_pfb_scan_totals(const int* __restrict__ flag, size_t rp, unsigned* tmp, int chunks, int K) {
  __shared__ unsigned sm[17];
  int b, c;
  if (!xcd_map(chunks, K, c, b)) return;
  pf_scan_totals(flag + (size_t)b * rp, rp, tmp + (size_t)b * chunks, c, sm);
}
__global__ void __launch_bounds__(1024) k_pfb_scan_offsets(unsigned* tmp, int chunks, const PfbItem* __restrict__ items, int K, int* res) {
  __shared__ unsigned sm[17];
  const int b = blockIdx.x;
  const unsigned total = pf_scan_offsets(tmp + (size_t)b * chunks, chunks, sm);
  if (threadIdx.x == 0) {
    res[b] = (int)total;
    if ((unsigned long long)total > items[b].out_pitch) atomicMin(&res[K], items[b].id);
  }
}
__global__ void __launch_bounds__(1024) k_pfb_scan_apply(const int* __restrict__ flag, size_t rp, const unsigned* __restrict__ tmp, int* pos, int chunks, int K) {
  __shared__ unsigned sm[17];
  int b, c;
  if (!xcd_map(chunks, K, c, b)) return;
  pf_scan_apply(flag + (size_t)b * rp, rp, tmp + (size_t)b * chunks, pos + (size_t)b * rp, c, sm);
}

// Emit: straight into the cloud's slot rows.  Nothing is written at or past the slot's pitch (such a cloud has raised the overflow word).
template <bool INTENSITY>
__global__ void __launch_bounds__(256) k_pfb_emit(const float* __restrict__ X, size_t rp, const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                  const int* __restrict__ flag, const int* __restrict__ pos, const PfGrid* __restrict__ grid, int downsample,
                                                  const PfbItem* __restrict__ items, int K, int nx, const PfbInt pi) {
  int b, bx;
  if (!xcd_map(nx, K, bx, b)) return;
  const int ds = downsample && grid[b].status == 0;
  const PfbItem it = items[b];
  const float* Xb = X + (size_t)b * 3 * rp;
  const unsigned* kb = keys + (size_t)b * rp;
  const unsigned* vb = vals + (size_t)b * rp;
  const int* fb = flag + (size_t)b * rp;
  const int* pb = pos + (size_t)b * rp;
  const float* Ib = nullptr;
  float* oi = nullptr;
  if constexpr (INTENSITY) { Ib = pi.in + (size_t)b * rp; oi = pi.out[b]; }
  const size_t end = std::min(rp, (size_t)(bx + 1) * RS_TILE);
  for (size_t i = (size_t)bx * RS_TILE + threadIdx.x; i < end; i += 256) {
    if (!fb[i]) continue;
    float sx, sy, sz, si = 0.f;
    pf_emit_point<INTENSITY>(Xb, rp, kb, vb, ds, i, sx, sy, sz, Ib, si);
    const size_t o = (size_t)pb[i];
    if (o < it.out_pitch) {
      it.out[o] = sx; it.out[it.out_pitch + o] = sy; it.out[2 * it.out_pitch + o] = sz;
      if constexpr (INTENSITY) oi[o] = si;
    }
  }
}
