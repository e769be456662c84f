// ndt_prefilter.hpp -- distance filter + VoxelGrid centroid down-sampling.
#pragma once
#include "ndt_types.hpp"

// ------------------------------------------------------------------------------------ prefilter (upstream of the path)
// PrefilteringNodelet::distance_filter + downsample (src/lidar_odometry/prefiltering_nodelet.cpp:137-181, parameters of
// launch/dlo_kitti.launch:30-36): keep points with near < |p| < far (f32 norm compared as double), then pcl::VoxelGrid
// centroid downsample (PCL 1.8 voxel_grid.hpp applyFilter, CentroidPoint / AccumulatorXYZ: f32 sums, divided by the
// count), output in ascending voxel index.  Same binning + stable sort machinery as the NDT target build.
// This file holds the per-point pieces and the exclusive scan; the kernels that run them are the segmented ones of ndt_prefilter_batch.hpp, for
// one cloud (mi355ndt_prefilter, mi355ndt_window_keyframe: a group of one) as for K.
// the gate: near < |p| < far (f32 norm compared as double, :168) and the finite test (VoxelGrid skips non-finite points: is_dense = false, :175)
__device__ __forceinline__ bool pf_gate(float x, float y, float z, int use_df, double dnear, double dfar) {
  bool ok = true;
  if (use_df) {
    const double d = (double)sqrtf((x * x + y * y) + z * z);         // p.getVector3fMap().norm() (:168)
    ok = d > dnear && d < dfar;                                      // NaN fails both compares
  }
  return ok && finite3(x, y, z);
}
// PrefilteringNodelet::vertical_angle_calibration (:183-220): the point, widened to f64, turned by `delta` about the normalised p x (0,0,1) and
// cast back to f32.  Eigen 3.3 restated operation for operation -- cross(), normalize() (squaredNorm; divided only when it is > 0, so a point on
// the z axis keeps a zero axis and is scaled by cos(delta)), AngleAxisd::toRotationMatrix() and the 3x3 product --, every operation rounded on
// its own, the terms that are zero kept: signed zeros come out as Eigen's.  sn, cs: sin(delta) and cos(delta), computed once on the host.
// The caller leaves a point with a non-finite coordinate as it is (the gate drops it), the base_link move's rule.
struct PfCal { int on; double sn, cs; };
__device__ __forceinline__ void pf_calibrate(float& x, float& y, float& z, double sn, double cs) {
  const double px = (double)x, py = (double)y, pz = (double)z;
  double a0 = py * 1.0 - pz * 0.0, a1 = pz * 0.0 - px * 1.0, a2 = px * 0.0 - py * 0.0;   // p.cross((0,0,1))
  const double s = (a0 * a0 + a1 * a1) + a2 * a2;
  if (s > 0.0) { const double r = sqrt(s); a0 /= r; a1 /= r; a2 /= r; }                    // normalize()
  const double s0 = sn * a0, s1 = sn * a1, s2 = sn * a2;                                   // sin_axis
  const double k = 1.0 - cs, c0 = k * a0, c1 = k * a1, c2 = k * a2;                        // cos1_axis
  double t = c0 * a1;
  const double r01 = t - s2, r10 = t + s2;
  t = c0 * a2;
  const double r02 = t + s1, r20 = t - s1;
  t = c1 * a2;
  const double r12 = t - s0, r21 = t + s0;
  const double r00 = c0 * a0 + cs, r11 = c1 * a1 + cs, r22 = c2 * a2 + cs;
  x = (float)((r00 * px + r01 * py) + r02 * pz);
  y = (float)((r10 * px + r11 * py) + r12 * pz);
  z = (float)((r20 * px + r21 * py) + r22 * pz);
}
// a thread's extremes (f2ord order) into the six words of its cloud: wave reduction, one atomic per wave and word
struct PfExt {
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  __device__ __forceinline__ void take(float x, float y, float z) {
    const int ox = f2ord(x), oy = f2ord(y), oz = f2ord(z);
    mn[0] = min(mn[0], ox); mx[0] = max(mx[0], ox);
    mn[1] = min(mn[1], oy); mx[1] = max(mx[1], oy);
    mn[2] = min(mn[2], oz); mx[2] = max(mx[2], oz);
  }
  __device__ __forceinline__ void commit(int* mm) {                  // (every lane of the wave calls it)
    for (int a = 0; a < 3; a++) {
      for (int o = 32; o > 0; o >>= 1) { mn[a] = min(mn[a], __shfl_xor(mn[a], o)); mx[a] = max(mx[a], __shfl_xor(mx[a], o)); }
      if ((threadIdx.x & 63) == 0) {
        if (mn[a] != INT_MAX) atomicMin(&mm[a], mn[a]);
        if (mx[a] != INT_MIN) atomicMax(&mm[3 + a], mx[a]);
      }
    }
  }
};

struct PfGrid { int min_b[3], mul1, mul2, status; float inv_leaf; };   // status: 0 ok, 1 empty, 2 index overflow

// the grid of one cloud from its six extremes
__device__ __forceinline__ PfGrid pf_make_grid(const int* __restrict__ mm, float leaf) {
  PfGrid g;
  memset(&g, 0, sizeof g);
  g.inv_leaf = 1.0f / leaf;
  if (mm[0] == INT_MAX) { g.status = 1; return g; }
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) { mn[a] = ord2f(mm[a]); mx[a] = ord2f(mm[3 + a]); }
  if (grid_too_big((mx[0] - mn[0]) * g.inv_leaf, (mx[1] - mn[1]) * g.inv_leaf, (mx[2] - mn[2]) * g.inv_leaf)) { g.status = 2; return g; }   // "Leaf size is too small": output = input
  int maxb[3];
  for (int a = 0; a < 3; a++) { g.min_b[a] = (int)floorf(mn[a] * g.inv_leaf); maxb[a] = (int)floorf(mx[a] * g.inv_leaf); }
  g.mul1 = maxb[0] - g.min_b[0] + 1;
  g.mul2 = g.mul1 * (maxb[1] - g.min_b[1] + 1);
  return g;
}

// the 31-bit voxel key of position i (0x7FFFFFFF: not binned -- past the cloud, dropped by the gate, or the cloud has no usable grid)
__device__ __forceinline__ unsigned pf_cell_key(const float* __restrict__ X, size_t pitch, int n, const unsigned char* __restrict__ keep,
                                                const PfGrid& g, size_t i) {
  unsigned cell = 0x7FFFFFFFu;
  if (i < (size_t)n && keep[i] && g.status == 0) {
    const int i0 = (int)(floorf(X[i] * g.inv_leaf) - (float)g.min_b[0]);
    const int i1 = (int)(floorf(X[pitch + i] * g.inv_leaf) - (float)g.min_b[1]);
    const int i2 = (int)(floorf(X[2 * pitch + i] * g.inv_leaf) - (float)g.min_b[2]);
    cell = (unsigned)(i0 + i1 * g.mul1 + i2 * g.mul2);
  }
  return cell;
}

// head of every occupied voxel's run (or, without down-sampling, every kept point)
__device__ __forceinline__ int pf_is_head(const unsigned* __restrict__ keys, const unsigned char* __restrict__ keep, int n, int downsample, size_t i) {
  if (downsample) return keys[i] != 0x7FFFFFFFu && (i == 0 || keys[i - 1] != keys[i]);
  return i < (size_t)n && keep[i];
}

// what the head at position i emits: the voxel's centroid -- the f32 sum of its points in input order, divided by (float)count -- or, without
// down-sampling, the point itself.  INTENSITY: XI, the cloud's row of the intensity plane, is walked beside the rows (AccumulatorIntensity: the
// same f32 sum in the same order, the same division) into si; without it neither is touched.
template <bool INTENSITY = false>
__device__ __forceinline__ void pf_emit_point(const float* __restrict__ X, size_t pitch, const unsigned* __restrict__ keys,
                                              const unsigned* __restrict__ vals, int downsample, size_t i, float& sx, float& sy, float& sz,
                                              const float* __restrict__ XI, float& si) {
  if (downsample) {
    const unsigned key = keys[i];
    sx = sy = sz = 0.f;
    if constexpr (INTENSITY) si = 0.f;
    int cnt = 0;
    for (size_t j = i; j < pitch && keys[j] == key; j++) {           // AccumulatorXYZ: xyz += p (f32), input order
      const unsigned pi = vals[j];
      sx += X[pi]; sy += X[pitch + pi]; sz += X[2 * pitch + pi];
      if constexpr (INTENSITY) si += XI[pi];
      cnt++;
    }
    const float fn = (float)cnt;
    sx /= fn; sy /= fn; sz /= fn;                                    // xyz / n
    if constexpr (INTENSITY) si /= fn;
  } else {
    sx = X[i]; sy = X[pitch + i]; sz = X[2 * pitch + i];
    if constexpr (INTENSITY) si = XI[i];
  }
}

// Exclusive prefix sum of n ints (the emit positions of the kept points / voxel heads): block totals of 4096-element chunks,
// one block scanning those totals, then every chunk scans itself again on top of its offset.
#define PF_SCAN_CHUNK 4096
// (the three bodies take the chunk they work on and the block's 17 words of LDS: the segmented scan of ndt_prefilter_batch.hpp runs them per cloud)
__device__ __forceinline__ void pf_scan_totals(const int* __restrict__ in, size_t n, unsigned* totals, int chunk, unsigned* sm) {
  const size_t i0 = (size_t)chunk * PF_SCAN_CHUNK + (size_t)threadIdx.x * 4;
  unsigned v = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) if (i0 + u < n) v += (unsigned)in[i0 + u];
  unsigned tot;
  (void)block_exscan<1024>(v, &tot, sm);
  if (threadIdx.x == 0) totals[chunk] = tot;
}
__device__ __forceinline__ unsigned pf_scan_offsets(unsigned* totals, int nchunks, unsigned* sm) {   // returns the sum of all chunks
  unsigned base = 0;
  for (int c0 = 0; c0 < nchunks; c0 += 1024) {
    const int c = c0 + threadIdx.x;
    const unsigned v = c < nchunks ? totals[c] : 0u;
    unsigned tot;
    const unsigned ex = block_exscan<1024>(v, &tot, sm);
    if (c < nchunks) totals[c] = base + ex;
    base += tot;
  }
  return base;
}
__device__ __forceinline__ void pf_scan_apply(const int* __restrict__ in, size_t n, const unsigned* __restrict__ offs, int* out, int chunk, unsigned* sm) {
  const size_t i0 = (size_t)chunk * PF_SCAN_CHUNK + (size_t)threadIdx.x * 4;
  unsigned e[4], v = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) { e[u] = i0 + u < n ? (unsigned)in[i0 + u] : 0u; v += e[u]; }
  unsigned tot;
  unsigned ex = block_exscan<1024>(v, &tot, sm) + offs[chunk];
#pragma unroll
  for (int u = 0; u < 4; u++) { if (i0 + u < n) out[i0 + u] = (int)ex; ex += e[u]; }
}
__global__ void __launch_bounds__(1024) k_pf_scan_totals(const int* __restrict__ in, size_t n, unsigned* totals) {
  __shared__ unsigned sm[17];
  pf_scan_totals(in, n, totals, (int)blockIdx.x, sm);
}
__global__ void __launch_bounds__(1024) k_pf_scan_offsets(unsigned* totals, int nchunks) {
  __shared__ unsigned sm[17];
  (void)pf_scan_offsets(totals, nchunks, sm);
}
__global__ void __launch_bounds__(1024) k_pf_scan_apply(const int* __restrict__ in, size_t n, const unsigned* __restrict__ offs, int* out) {
  __shared__ unsigned sm[17];
  pf_scan_apply(in, n, offs, out, (int)blockIdx.x, sm);
}
