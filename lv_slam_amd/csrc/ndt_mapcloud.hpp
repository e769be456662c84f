// ndt_mapcloud.hpp -- the global graph's map cloud: MapCloudGenerator::generate (src/global_graph/map_cloud_generator.cpp:17-55) on the device.
//
// Every keyframe's points moved by its pose, fed IN ORDER into pcl::octree::OctreePointCloud(resolution), the occupied voxel centres returned
// depth first (PCL 1.8 octree_pointcloud.hpp).  The CPU restatement, with the arithmetic step by step, is tools/map_cloud_ref.py.
//   k_mc_transform  points -> moved points (SoA, global order), finite flags, one f32 AABB per 4,096-point chunk
//   k_mc_box        ONE workgroup: the octree's box, grown point by point as addPointsFromInputCloud grows it (below)
//   k_mc_keys       64-bit Morton code of every point's leaf (non-finite: all ones, sorts last)
//   rs_pass x 6     stable LSD sort of the codes (ndt_segsort.hpp, the whole cloud one segment): low word first, carrying the high word
//   k_mc_heads, k_pf_scan_*, k_mc_emit   one centre per distinct code, in ascending code order = PCL's depth-first order
#pragma once
#include "ndt_types.hpp"

#define MC_CHUNK      4096           // points per AABB of k_mc_transform
#define MC_THREADS    256
#define MC_MAX_DEPTH  21             // 3 x 21 key bits = 63: the Morton code fits one 64-bit word, the all-ones sentinel above every code
#define MC_MAX_EVENTS (MC_MAX_DEPTH + 2)
#define MC_MAX_ITERS  (2 * MC_MAX_EVENTS + 4)

enum { MC_OK = 0, MC_EMPTY = 1, MC_DEPTH = 2, MC_ITERS = 3 };

struct McKf { const float* rows; unsigned start, pitch; };   // keyframe k: its x,y,z rows of `pitch` floats (staged or resident); global index of its first point
// The box after each point that changed it (the first finite point, then every point that grew it).  A point is keyed in the box of the
// last event at or before it, as addPointIdx keys it right after adoptBoundingBoxToPoint; `shift` = what the later growth levels add to
// that key (the old root hung below a new one as child (!upX << 2 | !upY << 1 | !upZ): +2^depth on every axis that grew downwards).
struct McEvent { double min[3]; unsigned pos, depth; unsigned shift[3], pad_; };
struct McBox { double min[3]; int depth, status, n_events, pad_; McEvent ev[MC_MAX_EVENTS]; };

// Morton interleave of three 21-bit keys: bit l of kx / ky / kz -> bit 3l+2 / 3l+1 / 3l (x the most significant of each level, the child
// index order of OctreeKey::getChildIdxWithDepthMask)
__device__ __forceinline__ unsigned long long mc_spread3(unsigned v) {
  unsigned long long x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ unsigned mc_compact3(unsigned long long x) {
  x &= 0x1249249249249249ull;
  x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
  x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
  x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
  x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
  x = (x ^ (x >> 32)) & 0x1fffffull;
  return (unsigned)x;
}

// One workgroup per 4,096 positions of the global order; position g < n is point g - kf[k].start of keyframe k.  Eigen's lazy Matrix4f *
// Vector4f with w = 1 (map_cloud_generator.cpp:31-35): ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3], every f32 step rounded (-ffp-contract=off).
// T: per keyframe the three upper rows of pose.cast<float>(), row-major.  aabb: per chunk the ordered-int extremes of its finite points
// (INT_MAX / INT_MIN: none).
__global__ void __launch_bounds__(MC_THREADS) k_mc_transform(const McKf* __restrict__ kf, int n_kf,
                                                             const float* __restrict__ T, int n, size_t pitch, float* X, unsigned char* fin, int* aabb) {
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  const int g0 = blockIdx.x * MC_CHUNK + threadIdx.x;
  int k = -1;
  if (g0 < n) {                                   // last keyframe whose first point is at or before g0 (empty keyframes share their successor's start)
    int lo = 0, hi = n_kf - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int)kf[mid].start <= g0) lo = mid; else hi = mid - 1; }
    k = lo;
  }
  for (int g = g0; g < blockIdx.x * MC_CHUNK + MC_CHUNK && g < (int)pitch; g += MC_THREADS) {
    float o[3] = {0.f, 0.f, 0.f};
    bool ok = false;
    if (g < n) {
      while (k + 1 < n_kf && (int)kf[k + 1].start <= g) k++;
      const McKf e = kf[k];
      const float* R = e.rows;
      const int j = g - (int)e.start;
      const float x = R[j], y = R[e.pitch + j], z = R[2 * (size_t)e.pitch + j];
      const float* M = T + 12 * (size_t)k;
#pragma unroll
      for (int a = 0; a < 3; a++) o[a] = ((M[4 * a] * x + M[4 * a + 1] * y) + M[4 * a + 2] * z) + M[4 * a + 3];
      ok = finite3(o[0], o[1], o[2]);             // addPointsFromInputCloud: isFinite of the moved point
    }
    X[g] = o[0]; X[pitch + g] = o[1]; X[2 * pitch + g] = o[2];
    fin[g] = ok ? 1 : 0;
    if (ok)
      for (int a = 0; a < 3; a++) { const int v = f2ord(o[a]); mn[a] = min(mn[a], v); mx[a] = max(mx[a], v); }
  }
  __shared__ int sm[MC_THREADS / 64][6];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int a = 0; a < 3; a++)
    for (int s = 32; s > 0; s >>= 1) { mn[a] = min(mn[a], __shfl_xor(mn[a], s)); mx[a] = max(mx[a], __shfl_xor(mx[a], s)); }
  if (lane == 0) for (int a = 0; a < 3; a++) { sm[w][a] = mn[a]; sm[w][3 + a] = mx[a]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int t = threadIdx.x;
    int v = sm[0][t];
    for (int w2 = 1; w2 < MC_THREADS / 64; w2++) v = t < 3 ? min(v, sm[w2][t]) : max(v, sm[w2][t]);
    aabb[6 * (size_t)blockIdx.x + t] = v;
  }
}

// The box as OctreePointCloud keeps it, for lane 0 of k_mc_box (f64 throughout, eps = (double)FLT_EPSILON).
struct McState { double min[3], max[3], r; int depth, defined; unsigned long long down[3]; };
// adoptBoundingBoxToPoint(q): the first point defines the box (then getKeyBitSize with leaf_count_ == 0); while q lies outside
// [min, max) the tree gains a level on top.  false: the depth passed MC_MAX_DEPTH.
__device__ bool mc_adopt(McState& s, const double q[3]) {
  const double eps = (double)FLT_EPSILON;
  if (!s.defined) {
    unsigned mk = 2;
    for (int a = 0; a < 3; a++) {
      s.min[a] = q[a] - s.r / 2; s.max[a] = q[a] + s.r / 2;
      mk = max(mk, (unsigned)((s.max[a] - s.min[a]) / s.r));
    }
    s.depth = min(32, (int)ceil(log((double)mk) / log(2.0) - eps));
    const double side = (double)(1ull << s.depth) * s.r - eps;
    for (int a = 0; a < 3; a++) {
      const double over = (side - (s.max[a] - s.min[a])) / 2.0;
      s.min[a] -= over; s.max[a] += over;
    }
    s.defined = 1;
  }
  for (;;) {
    bool viol = false, up[3];
    for (int a = 0; a < 3; a++) { up[a] = q[a] >= s.max[a]; viol = viol || q[a] < s.min[a] || up[a]; }
    if (!viol) return true;
    const double side = (double)(1ull << s.depth) * s.r;
    for (int a = 0; a < 3; a++) if (!up[a]) { s.min[a] -= side; s.down[a] += 1ull << s.depth; }
    s.depth++;
    if (s.depth > MC_MAX_DEPTH) return false;
    const double side2 = (double)(1ull << s.depth) * s.r - eps;
    for (int a = 0; a < 3; a++) s.max[a] = s.min[a] + side2;
  }
}

// One workgroup, no host round trip: from a cursor, (1) the first chunk whose AABB leaves the current box (exact: the AABB's extremes are
// f32 values of its own points, so a chunk wholly past the cursor that passes this test holds a violating point), (2) that chunk's first
// violating point at or after the cursor, (3) lane 0 grows the box for it, (4) the cursor moves past it.  Every violating point but the first
// adds a level, so there are at most MC_MAX_EVENTS rounds, each reading N / 4,096 boxes and one chunk; a round whose chunk holds the cursor
// may find nothing there (its AABB covers points before the cursor) and moves on.  The loop is bounded and ends in out->status.
__global__ void __launch_bounds__(MC_THREADS) k_mc_box(const float* __restrict__ X, size_t pitch, const unsigned char* __restrict__ fin,
                                                       const int* __restrict__ aabb, int n, double r, McBox* out) {
  __shared__ double s_min[3], s_max[3];
  __shared__ int s_defined, s_cursor, s_best, s_stop;
  __shared__ McEvent s_ev[MC_MAX_EVENTS];
  __shared__ int s_nev, s_status;
  McState st;                                     // lane 0's
  const int tid = threadIdx.x;
  if (tid == 0) {
    st.r = r; st.depth = 0; st.defined = 0;
    for (int a = 0; a < 3; a++) { st.min[a] = st.max[a] = 0.0; st.down[a] = 0; s_min[a] = s_max[a] = 0.0; }
    s_defined = 0; s_cursor = 0; s_nev = 0; s_status = MC_OK; s_stop = 0;
  }
  const int nchunks = (n + MC_CHUNK - 1) / MC_CHUNK;
  int it = 0;
  for (; it < MC_MAX_ITERS; it++) {
    __syncthreads();
    const int cursor = s_cursor;
    if (s_stop || cursor >= n) break;
    const bool defined = s_defined != 0;
    const double bmin[3] = {s_min[0], s_min[1], s_min[2]}, bmax[3] = {s_max[0], s_max[1], s_max[2]};
    // (1) first candidate chunk, 256 chunks per step
    int cand = INT_MAX;
    for (int cb = cursor / MC_CHUNK; cb < nchunks; cb += MC_THREADS) {
      if (tid == 0) s_best = INT_MAX;
      __syncthreads();
      const int c = cb + tid;
      if (c < nchunks) {
        const int* A = aabb + 6 * (size_t)c;
        bool v = false;
        if (A[0] != INT_MAX) {
          v = !defined;
          for (int a = 0; a < 3; a++) v = v || (double)ord2f(A[a]) < bmin[a] || (double)ord2f(A[3 + a]) >= bmax[a];
        }
        if (v) atomicMin(&s_best, c);
      }
      __syncthreads();
      cand = s_best;
      __syncthreads();
      if (cand != INT_MAX) break;
    }
    if (cand == INT_MAX) break;                   // no point past the cursor leaves the box
    // (2) its first violating point at or after the cursor
    const int p0 = max(cursor, cand * MC_CHUNK), p1 = min(n, (cand + 1) * MC_CHUNK);
    int hit = INT_MAX;
    for (int pb = p0; pb < p1; pb += MC_THREADS) {
      if (tid == 0) s_best = INT_MAX;
      __syncthreads();
      const int i = pb + tid;
      if (i < p1 && fin[i]) {
        bool v = !defined;
        for (int a = 0; a < 3; a++) { const double q = (double)X[a * pitch + i]; v = v || q < bmin[a] || q >= bmax[a]; }
        if (v) atomicMin(&s_best, i);
      }
      __syncthreads();
      hit = s_best;
      __syncthreads();
      if (hit != INT_MAX) break;
    }
    if (tid == 0) {
      if (hit == INT_MAX) s_cursor = p1;         // only points before the cursor were outside: go on behind this chunk
      else {
        // (3) the growth, in one lane
        const double q[3] = {(double)X[hit], (double)X[pitch + hit], (double)X[2 * pitch + hit]};
        const bool ok = mc_adopt(st, q);
        McEvent& e = s_ev[s_nev];
        for (int a = 0; a < 3; a++) { e.min[a] = st.min[a]; e.shift[a] = (unsigned)st.down[a]; s_min[a] = st.min[a]; s_max[a] = st.max[a]; }
        e.pos = (unsigned)hit; e.depth = (unsigned)st.depth; e.pad_ = 0;
        s_nev++;
        s_defined = 1;
        s_cursor = hit + 1;                       // (4)
        if (!ok) { s_status = MC_DEPTH; s_stop = 1; }
        else if (s_nev == MC_MAX_EVENTS) s_stop = 1;   // (cannot happen below the depth limit: every event after the first adds a level)
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    McBox b;
    memset(&b, 0, sizeof b);
    b.status = s_status;
    if (s_status == MC_OK && (it == MC_MAX_ITERS || (s_stop && s_cursor < n))) b.status = MC_ITERS;
    if (s_nev == 0 && b.status == MC_OK) b.status = MC_EMPTY;
    b.depth = st.depth;
    b.n_events = s_nev;
    for (int a = 0; a < 3; a++) b.min[a] = st.min[a];
    for (int e = 0; e < s_nev; e++) {
      b.ev[e] = s_ev[e];
      for (int a = 0; a < 3; a++) b.ev[e].shift[a] = (unsigned)(st.down[a] - s_ev[e].shift[a]);   // down so far -> what later levels add
    }
    *out = b;
  }
}

// The leaf of every finite point: key = (unsigned)((q - min) / r) per axis (genOctreeKeyforPoint, an f64 division) in the box of its event,
// its low `depth` bits (createLeafRecursive's depth mask), plus the later levels' shift; then the Morton code of the final tree.
__global__ void __launch_bounds__(256) k_mc_keys(const float* __restrict__ X, size_t pitch, const unsigned char* __restrict__ fin,
                                                 const McBox* __restrict__ box, double r, unsigned* klo, unsigned* khi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int)pitch) return;
  unsigned long long code = ~0ull;
  if (fin[i] && box->status == MC_OK) {
    const int ne = box->n_events;
    int e = 0;
    while (e + 1 < ne && box->ev[e + 1].pos <= (unsigned)i) e++;
    const McEvent& ev = box->ev[e];
    const unsigned mask = ev.depth >= 32 ? 0xFFFFFFFFu : (1u << ev.depth) - 1u;
    unsigned k[3];
#pragma unroll
    for (int a = 0; a < 3; a++) k[a] = ((unsigned)(((double)X[a * pitch + i] - ev.min[a]) / r) & mask) + ev.shift[a];
    code = (mc_spread3(k[0]) << 2) | (mc_spread3(k[1]) << 1) | mc_spread3(k[2]);
  }
  klo[i] = (unsigned)code;
  khi[i] = (unsigned)(code >> 32);
}

// first position of every distinct code (the sentinel excluded)
__global__ void __launch_bounds__(256) k_mc_heads(const unsigned* __restrict__ lo, const unsigned* __restrict__ hi, size_t pitch, int* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int)pitch) return;
  const bool none = lo[i] == 0xFFFFFFFFu && hi[i] == 0xFFFFFFFFu;
  flag[i] = !none && (i == 0 || lo[i - 1] != lo[i] || hi[i - 1] != hi[i]);
}

// genLeafNodeCenterFromOctreeKey: (float)(((double)key + 0.5) * r + min) per axis, x,y,z records at the scanned positions
__global__ void __launch_bounds__(256) k_mc_emit(const unsigned* __restrict__ lo, const unsigned* __restrict__ hi, const int* __restrict__ flag,
                                                 const int* __restrict__ pos, size_t pitch, const McBox* __restrict__ box, double r, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int)pitch || !flag[i]) return;
  const unsigned long long code = ((unsigned long long)hi[i] << 32) | lo[i];
  const unsigned k[3] = {mc_compact3(code >> 2), mc_compact3(code >> 1), mc_compact3(code)};
  const size_t o = 3 * (size_t)pos[i];
#pragma unroll
  for (int a = 0; a < 3; a++) out[o + a] = (float)(((double)k[a] + 0.5) * r + box->min[a]);
}
