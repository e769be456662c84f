// ndt_keyframe.hpp -- the window map of the global graph on the device: GlobalGraphNodelet::cloud_callback's window accumulation and
// down-sampling (src/global_graph/global_graph_nodelet.cpp:202-244).
//
// The scans between two keyframe decisions are moved into the window's first frame (pcl::transformPointCloud<PointT, double>, :241), appended
// in scan order (:242), and the whole window goes through pcl::VoxelGrid(leaf) when it closes (:214-218).  The CPU restatement, with the
// arithmetic step by step, is tools/window_map_ref.py.
//   k_kf_window   ONE pass over the window: scan rows -> moved points (and intensity), SoA in window order, keep flags, f32 extremes
//   k_pfb_grid, k_pfb_keys, rs_pass x 3, k_pfb_heads, k_pfb_scan_*   the prefilter's segmented VoxelGrid chain (ndt_prefilter_batch.hpp), the
//                 window its one cloud; the grid's status ("leaf too small") is decided and consumed on the device
//   k_kf_emit     one centroid per occupied voxel, x, y, z and intensity, straight into the keyframe's own rows
#pragma once
#include "ndt_types.hpp"
#include "ndt_prefilter.hpp"

#define KF_CHUNK   1024              // window positions per workgroup of k_kf_window (four per lane)
#define KF_THREADS 256

// scan k: its x, y, z rows of `pitch` floats; the window index of its first point; its intensity row (null: the scan carries none, and a window
// with an intensity reads +0 for its points)
struct KfScan { const float* rows; unsigned start, pitch; const float* irow; };

// One workgroup per 1,024 positions of the window; position g < n is point g - sc[k].start of scan k (binary search once per lane, then a
// walk, as k_mc_transform does).  PCL 1.8 transformPointCloud with a double matrix: per coordinate
//   (float)(((T(a,0) x + T(a,1) y) + T(a,2) z) + T(a,3)),  x, y, z widened to f64 first, ONE rounding to f32 at the end (-ffp-contract=off).
// T: per scan the three upper rows of (w_odom.inverse() * odom_k).matrix(), row-major f64; scan 0 is the window's own frame and is taken as
// it is (:206, :232).  A point with a non-finite coordinate is not moved (PCL skips it in a non-dense cloud) and is not kept; neither is a
// point the move pushes out of f32's range: VoxelGrid drops both.  Positions n .. pitch are written as zeros, not kept.
// mm: the ordered-int extremes of the kept points, reduced per wave before one atomic per wave and word (PfExt's pattern).
__global__ void __launch_bounds__(KF_THREADS) k_kf_window(const KfScan* __restrict__ sc, int n_scans, const double* __restrict__ T, int n, size_t pitch,
                                                          int ch, float* X, unsigned char* keep, int* mm) {
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  const int g0 = blockIdx.x * KF_CHUNK + threadIdx.x;
  int k = 0;
  if (g0 < n) {                                   // last scan whose first point is at or before g0 (empty scans share their successor's start)
    int lo = 0, hi = n_scans - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int)sc[mid].start <= g0) lo = mid; else hi = mid - 1; }
    k = lo;
  }
  for (int g = g0; g < blockIdx.x * KF_CHUNK + KF_CHUNK && g < (int)pitch; g += KF_THREADS) {
    float o[3] = {0.f, 0.f, 0.f}, w = 0.f;
    bool ok = false;
    if (g < n) {
      while (k + 1 < n_scans && (int)sc[k + 1].start <= g) k++;
      const KfScan e = sc[k];
      const int j = g - (int)e.start;
      const float x = e.rows[j], y = e.rows[e.pitch + j], z = e.rows[2 * (size_t)e.pitch + j];
      if (ch == 4 && e.irow) w = e.irow[j];
      o[0] = x; o[1] = y; o[2] = z;
      ok = finite3(x, y, z);
      if (ok && k > 0) {
        const double* M = T + 12 * (size_t)k;
        const double xd = (double)x, yd = (double)y, zd = (double)z;
#pragma unroll
        for (int a = 0; a < 3; a++) o[a] = (float)(((M[4 * a] * xd + M[4 * a + 1] * yd) + M[4 * a + 2] * zd) + M[4 * a + 3]);
        ok = finite3(o[0], o[1], o[2]);
      }
    }
    X[g] = o[0]; X[pitch + g] = o[1]; X[2 * pitch + g] = o[2];
    if (ch == 4) X[3 * pitch + g] = w;
    keep[g] = ok ? 1 : 0;
    if (ok)
      for (int a = 0; a < 3; a++) { const int v = f2ord(o[a]); mn[a] = min(mn[a], v); mx[a] = max(mx[a], v); }
  }
  for (int a = 0; a < 3; a++) {
    for (int s = 32; s > 0; s >>= 1) { mn[a] = min(mn[a], __shfl_xor(mn[a], s)); mx[a] = max(mx[a], __shfl_xor(mx[a], s)); }
    if ((threadIdx.x & 63) == 0) {
      if (mn[a] != INT_MAX) atomicMin(&mm[a], mn[a]);
      if (mx[a] != INT_MIN) atomicMax(&mm[3 + a], mx[a]);
    }
  }
}

// One lane per voxel head (or, without down-sampling, per kept point).  CentroidPoint<PointXYZI>: AccumulatorXYZ and AccumulatorIntensity add
// the points of the voxel in f32, in input order (the stable sort keeps it), and divide by float(n).  The sums are order-bound, so a run
// stays with its one lane however long it is.  Rows past the m emitted points, up to the keyframe's pitch, are zeroed here.
// downsample: leaf > 0; a window whose grid says the leaf is too small is emitted as it is (k_pfb_emit's rule).
__global__ void __launch_bounds__(256) k_kf_emit(const float* __restrict__ X, size_t pitch, const unsigned* __restrict__ keys,
                                                 const unsigned* __restrict__ vals, const int* __restrict__ flag, const int* __restrict__ pos,
                                                 const PfGrid* __restrict__ grid, int downsample, int ch, float* out, size_t out_pitch, size_t m) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pitch) return;
  downsample = downsample && grid->status == 0;
  if (i >= m && i < out_pitch)
    for (int c = 0; c < ch; c++) out[c * out_pitch + i] = 0.f;
  if (!flag[i]) return;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (downsample) {
    const unsigned key = keys[i];
    int cnt = 0;
    for (size_t j = i; j < pitch && keys[j] == key; j++) {
      const unsigned pi = vals[j];
      s[0] += X[pi]; s[1] += X[pitch + pi]; s[2] += X[2 * pitch + pi];
      if (ch == 4) s[3] += X[3 * pitch + pi];
      cnt++;
    }
    const float fn = (float)cnt;
    for (int c = 0; c < 4; c++) s[c] /= fn;
  } else {
    s[0] = X[i]; s[1] = X[pitch + i]; s[2] = X[2 * pitch + i];
    if (ch == 4) s[3] = X[3 * pitch + i];
  }
  const size_t o = (size_t)pos[i];
  if (o >= m) return;                             // (cannot happen: pos is the scan of flag, m its total)
  for (int c = 0; c < ch; c++) out[c * out_pitch + o] = s[c];
}
