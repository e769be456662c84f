// ndt_gicp.hpp -- the three device stages of pclomp::GeneralizedIterativeClosestPoint (include/ndt_omp/gicp_omp.h, gicp_omp_impl.hpp), the
// registration the loop-closure factory hands out for registration_method = GICP_OMP (src/global_graph/registrations.cpp:43-53).  The BFGS
// optimiser and the outer loop are the host's (gicp_bfgs.hpp, ndt_host_gicp.hpp); tools/gicp_ref.py restates all of it.
//
// 1. k_gc_cov -- computeCovariances (:60-133).  Per searchable point (three finite coordinates) the k nearest searchable points, itself
//    included, ascending by (d2, point id): d2 = (dx*dx + dy*dy) + dz*dz in f32 as in k_ol_knn; the id breaks ties (the engine's rule: FLANN's
//    is not observable).  In that order mean += (double)pt.x ..., cov(r,c) += (double)(pt.r * pt.c) over the lower triangle (the product f32,
//    as the reference writes it); mean /= k; cov(r,c) = cov(r,c) / k - mean[r] * mean[c]; eigen_sym3 (the voxel build's cyclic Jacobi, where
//    the reference runs Eigen::JacobiSVD); with c0, c1, c2 the eigenvectors by descending eigenvalue (equal ones in column order),
//    cov(r,c) = (c0[r]*c0[c] + c1[r]*c1[c]) + (eps*c2[r])*c2[c].  Nine f64 per point, SoA: cov[e * pitch + id], e = 3 r + c.  A non-finite
//    point keeps the zeros the host wrote.
//    The search is the outlier stage's (knn_fill, ndt_outlier.hpp): OlList with its id column, [slot][lane] in LDS, one wave per workgroup,
//    queries in cell order over the cloud's lattice (fit_rings with the list's worst entry as `best`: every point of an unvisited ring is
//    strictly further than that, so no tie is lost), or exhaustive over LDS tiles for a cloud whose lattice gave GRID_CAP.  One kernel, the
//    path taken by the lattice's status.  LDS per workgroup: CAP * 64 * 8 B of list + 3 KB of tile = 19 KB (CAP 32) / 35 KB (CAP 64).
// 2. k_gc_match -- the correspondence loop (:415-466).  Source point i, in input order: q = T (G p), two f32 products, each coordinate
//    ((a*x + b*y) + c*z) + d (w = 1); exact 1-NN over the target's index, a tie to the lower point id; matched iff (double)d2 < threshold^2;
//    M_i = (R C1_i R' + C2_j)^-1 in f64, R = the 3x3 block of the f64 product T G (the host forms it, k ascending), in this order:
//      A(r,c)    = (R(r,0)*C1(0,c) + R(r,1)*C1(1,c)) + R(r,2)*C1(2,c)
//      temp(r,c) = ((A(r,0)*R(c,0) + A(r,1)*R(c,1)) + A(r,2)*R(c,2)) + C2(r,c)
//      M         = cofactors of temp over det = (cof(0,0)*temp(0,0) + cof(1,0)*temp(1,0)) + cof(2,0)*temp(2,0), each entry cof * (1 / det)
//                  (ndt_math.hpp mat3_inverse: Eigen 3.3 compute_inverse<Matrix3d>)
//    idx[i] = the target id or -1, M SoA (zeros where unmatched), *m += matched (an integer atomic).  Nothing is compacted: the reference's
//    order of matches is whatever OpenMP produced.  A non-finite source point, or one whose q is not finite, matches nothing.
// 3. k_gc_cost + k_gc_cost_final -- operator(), df, fdf (:255-378): thirteen f64 sums over the matched points,
//      pp = Tx p (f32), res_a = (double)(pp_a - tgt_a) (an f32 subtraction), temp = M res, f += res . temp, g_t += temp,
//      Rm(r,c) += (double)(B p)_r * temp_c, B = the base transformation.
//    The tree is fixed by the source index alone: 256 consecutive points per chunk -- 64 lanes by shuffle-xor 32, 16, ... 1, then the chunk's
//    four wave sums in wave order -- then chunk c into slot c % 256 in ascending c, then the 256 slots by halving (slot t += slot t + s,
//    s = 128 ... 1).  No float atomics.  The record (13 sums, m) is written into mapped host memory.  The two halves of the tree are
//    templates on the number of sums (gc_chunk_tree, gc_slot_tree): the ICP step (ndt_icp.hpp) sums sixteen over the same tree.
// 4. k_gc_match_batch + k_gc_cost_batch + k_gc_cost_final_batch -- stages 2 and 3 for every slot of mi355ndt_gicp_batch_align that waits for
//    one, in one round.  The per-thread bodies of 2 and 3 are __device__ functions (gc_match_body, gc_cost_body, gc_final_body) which the
//    single-pair and the batch kernels both instantiate; see section 4 below.
#pragma once
#include "ndt_types.hpp"
#include "ndt_math.hpp"
#include "ndt_fitness.hpp"
#include "ndt_kffitness.hpp"
#include "ndt_outlier.hpp"

#define GC_CHUNK 256
#define GC_SUMS  13
#define GC_REC   16                      // doubles of the result record: 13 sums, m, two spare

// ---- 1. covariances ------------------------------------------------------------------------------------------
template <int CAP>
__global__ void __launch_bounds__(OL_LANES) k_gc_cov(KfiView v, int K, double eps, double* __restrict__ cov) {
  __shared__ float lst[CAP][OL_LANES];
  __shared__ unsigned lid[CAP][OL_LANES];
  const float* rows = v.rows;
  const size_t pitch = v.pitch;
  OlList<CAP, true> list;
  list.init(lst, K, lid);
  const unsigned j = blockIdx.x * OL_LANES + threadIdx.x;
  const float inf = __int_as_float(0x7f800000);
  unsigned id;
  const bool live = v.gd->status == GRID_OK ? knn_fill<true, false>(v, j, inf, list, id) : knn_fill<false, false>(v, j, inf, list, id);
  if (!live || !list.full()) return;
  double mean[3] = {0.0, 0.0, 0.0}, c00 = 0.0, c10 = 0.0, c11 = 0.0, c20 = 0.0, c21 = 0.0, c22 = 0.0;
  list.ascending([&](float, unsigned t) {
    const float x = rows[t], y = rows[pitch + t], z = rows[2 * pitch + t];
    mean[0] += (double)x; mean[1] += (double)y; mean[2] += (double)z;
    c00 += (double)(x * x);
    c10 += (double)(y * x); c11 += (double)(y * y);
    c20 += (double)(z * x); c21 += (double)(z * y); c22 += (double)(z * z);
  });
  const double kd = (double)K;
  for (int a = 0; a < 3; a++) mean[a] = mean[a] / kd;
  double A[9], ev[3], V[9];
  A[0] = c00 / kd - mean[0] * mean[0];
  A[3] = c10 / kd - mean[1] * mean[0]; A[4] = c11 / kd - mean[1] * mean[1];
  A[6] = c20 / kd - mean[2] * mean[0]; A[7] = c21 / kd - mean[2] * mean[1]; A[8] = c22 / kd - mean[2] * mean[2];
  A[1] = A[3]; A[2] = A[6]; A[5] = A[7];
  ndtm::eigen_sym3(A, ev, V);
  // the columns by descending eigenvalue, equal ones in the order they have (a zero matrix -- k = 1 -- keeps x, y, z: diag(1, 1, eps))
  int o0 = 0, o1 = 1, o2 = 2, t;
  if (ev[o1] > ev[o0]) { t = o0; o0 = o1; o1 = t; }
  if (ev[o2] > ev[o1]) { t = o1; o1 = o2; o2 = t; }
  if (ev[o1] > ev[o0]) { t = o0; o0 = o1; o1 = t; }
  double c0[3], c1[3], c2[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double a0 = V[r * 3], a1 = V[r * 3 + 1], a2 = V[r * 3 + 2];
    c0[r] = o0 == 0 ? a0 : (o0 == 1 ? a1 : a2);
    c1[r] = o1 == 0 ? a0 : (o1 == 1 ? a1 : a2);
    c2[r] = o2 == 0 ? a0 : (o2 == 1 ? a1 : a2);
  }
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) cov[(size_t)(3 * r + c) * pitch + id] = (c0[r] * c0[c] + c1[r] * c1[c]) + (eps * c2[r]) * c2[c];
}

// ---- 2. matching and Mahalanobis matrices -----------------------------------------------------------------------
struct GcMatch {
  float G[16], T[16];                              // the guess and transformation_, column-major
  double R[9];                                     // the 3x3 block of the f64 product T G, row-major
  double thr2;                                     // corr_dist_threshold^2
  float range;                                     // nothing further than this (slightly above thr2, f32) can match: the ring walk may stop there
};

// a 1-NN candidate: the nearer point, the lower id on a tie
__device__ __forceinline__ void gc_nearer(float d2, unsigned id, float& best, unsigned& bid) {
  if (d2 < best || (d2 == best && id < bid)) { best = d2; bid = id; }
}

// the per-thread body of the matching kernels: source points chunk * 256 .. + 255 of one cloud.  The WHOLE workgroup calls it (fit_tiles and
// the ballot); k_gc_match and k_gc_match_batch instantiate this one copy, which is what makes their bytes equal.
__device__ __forceinline__ void gc_match_body(const float* __restrict__ src, size_t spitch, int n_src, const KfiView& tgt, const GcMatch& a,
                                              const double* __restrict__ c1, const double* __restrict__ c2,
                                              int* __restrict__ idx, double* __restrict__ maha, int* m, int chunk) {
  const GridDesc& g = *tgt.gd;
  const size_t tpitch = tgt.pitch;
  const int i = chunk * 256 + threadIdx.x;
  float q[3] = {0.f, 0.f, 0.f};
  bool live = false;
  if (i < n_src) {
    const float px = src[i], py = src[spitch + i], pz = src[2 * spitch + i];
    float u[3];
#pragma unroll
    for (int r = 0; r < 3; r++) u[r] = ((a.G[0 * 4 + r] * px + a.G[1 * 4 + r] * py) + a.G[2 * 4 + r] * pz) + a.G[3 * 4 + r];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = ((a.T[0 * 4 + r] * u[0] + a.T[1 * 4 + r] * u[1]) + a.T[2 * 4 + r] * u[2]) + a.T[3 * 4 + r];
    live = finite3(px, py, pz) && finite3(q[0], q[1], q[2]);
  }
  float best = __int_as_float(0x7f800000);
  unsigned bid = 0xFFFFFFFFu;
  if (g.status == GRID_OK) {
    const float* X = tgt.sorted;
    const unsigned* ids = tgt.ids;
    if (live)
      fit_rings(q, g, tgt.words, tgt.runs, 1 << 30, a.range, best, [&](unsigned j0, unsigned j1) {
        for (unsigned t = j0; t < j1; t++) gc_nearer(fit_d2(q, X[t], X[tpitch + t], X[2 * tpitch + t]), ids[t], best, bid);
      });
  } else if (g.status == GRID_CAP) {               // no lattice: exhaustive (a target without a finite point: nothing)
    fit_tiles<256>(tgt.rows, tpitch, tgt.n, [&](float x, float y, float z, unsigned t) {
      if (live) gc_nearer(fit_d2(q, x, y, z), t, best, bid);
    });
  }
  const bool matched = live && bid != 0xFFFFFFFFu && (double)best < a.thr2;
  const unsigned long long b = __ballot(matched);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(m, __popcll(b));
  if (i >= n_src) return;
  idx[i] = matched ? (int)bid : -1;
  double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (matched) {
    double C1[9], A[9], t[9];
#pragma unroll
    for (int e = 0; e < 9; e++) C1[e] = c1[(size_t)e * spitch + i];
    ndtm::mat3_mul(a.R, C1, A);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        t[3 * r + c] = ((A[3 * r] * a.R[3 * c] + A[3 * r + 1] * a.R[3 * c + 1]) + A[3 * r + 2] * a.R[3 * c + 2]) + c2[(size_t)(3 * r + c) * tpitch + bid];
    ndtm::mat3_inverse(t, M);
  }
#pragma unroll
  for (int e = 0; e < 9; e++) maha[(size_t)e * spitch + i] = M[e];
}

__global__ void __launch_bounds__(256) k_gc_match(const float* __restrict__ src, size_t spitch, int n_src, KfiView tgt, GcMatch a,
                                                  const double* __restrict__ c1, const double* __restrict__ c2,
                                                  int* __restrict__ idx, double* __restrict__ maha, int* m) {
  gc_match_body(src, spitch, n_src, tgt, a, c1, c2, idx, maha, m, (int)blockIdx.x);
}

// ---- the fixed-order tree of NS f64 sums (the GICP cost: 13; the ICP step, ndt_icp.hpp: 16) -------------------------------
// gc_chunk_tree: a chunk's 256 lanes -> part[chunk][NS]: 64 lanes by shuffle-xor 32, 16, ... 1, then the four wave sums in wave order.  The
// WHOLE workgroup of GC_CHUNK threads calls it (a lane without a term brings zeros).
template <int NS>
__device__ __forceinline__ void gc_chunk_tree(double (&v)[NS], double* __restrict__ part, int chunk) {
  __shared__ double ws[GC_CHUNK / 64][NS];
#pragma unroll
  for (int k = 0; k < NS; k++)
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < NS; k++) ws[threadIdx.x >> 6][k] = v[k];
  __syncthreads();
  if (threadIdx.x < NS) {
    const int k = threadIdx.x;
    part[(size_t)chunk * NS + k] = ((ws[0][k] + ws[1][k]) + ws[2][k]) + ws[3][k];
  }
}
// gc_slot_tree: one cloud's chunks -> rec[0 .. NS - 1], by one workgroup of 256: chunk c into slot c % 256 in ascending c, then the 256
// slots by halving
template <int NS>
__device__ __forceinline__ void gc_slot_tree(const double* __restrict__ part, int n_chunks, double* rec) {
  __shared__ double sm[256];
  for (int k = 0; k < NS; k++) {
    double s = 0.0;
    for (int c = threadIdx.x; c < n_chunks; c += 256) s += part[(size_t)c * NS + k];
    __syncthreads();
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) rec[k] = sm[0];
  }
}

// ---- 3. cost sweep ---------------------------------------------------------------------------------------------
struct GcCost { float Tx[16], B[16]; };            // applyState(base, x) and the base transformation, column-major

// the per-thread body of the cost kernels: chunk `chunk` of one cloud -> part[chunk][13]; one copy behind k_gc_cost and k_gc_cost_batch
__device__ __forceinline__ void gc_cost_body(const float* __restrict__ src, size_t spitch, int n_src, const float* __restrict__ tgt, size_t tpitch,
                                             const int* __restrict__ idx, const double* __restrict__ maha, const GcCost& a, double* __restrict__ part,
                                             int chunk) {
  const int i = chunk * GC_CHUNK + threadIdx.x;
  double v[GC_SUMS];
#pragma unroll
  for (int k = 0; k < GC_SUMS; k++) v[k] = 0.0;
  const int j = i < n_src ? idx[i] : -1;
  if (j >= 0) {
    const float px = src[i], py = src[spitch + i], pz = src[2 * spitch + i];
    const float tg[3] = {tgt[j], tgt[tpitch + j], tgt[2 * tpitch + j]};
    double res[3], bp[3], M[9], temp[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const float pp = ((a.Tx[0 * 4 + r] * px + a.Tx[1 * 4 + r] * py) + a.Tx[2 * 4 + r] * pz) + a.Tx[3 * 4 + r];
      res[r] = (double)(pp - tg[r]);
      bp[r] = (double)(((a.B[0 * 4 + r] * px + a.B[1 * 4 + r] * py) + a.B[2 * 4 + r] * pz) + a.B[3 * 4 + r]);
    }
#pragma unroll
    for (int e = 0; e < 9; e++) M[e] = maha[(size_t)e * spitch + i];
#pragma unroll
    for (int r = 0; r < 3; r++) temp[r] = (M[3 * r] * res[0] + M[3 * r + 1] * res[1]) + M[3 * r + 2] * res[2];
    v[0] = (res[0] * temp[0] + res[1] * temp[1]) + res[2] * temp[2];
#pragma unroll
    for (int c = 0; c < 3; c++) v[1 + c] = temp[c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) v[4 + 3 * r + c] = bp[r] * temp[c];
  }
  gc_chunk_tree<GC_SUMS>(v, part, chunk);
}

__global__ void __launch_bounds__(GC_CHUNK) k_gc_cost(const float* __restrict__ src, size_t spitch, int n_src, const float* __restrict__ tgt, size_t tpitch,
                                                      const int* __restrict__ idx, const double* __restrict__ maha, GcCost a, double* __restrict__ part) {
  gc_cost_body(src, spitch, n_src, tgt, tpitch, idx, maha, a, part, (int)blockIdx.x);
}

// one cloud's tree over its chunks' partials, by one workgroup of 256: rec[0 .. 12] = the sums
__device__ __forceinline__ void gc_final_body(const double* __restrict__ part, int n_chunks, double* rec) { gc_slot_tree<GC_SUMS>(part, n_chunks, rec); }

// the chunks' partials -> the record: rec[0 .. 12] = the sums, rec[13] = m
__global__ void __launch_bounds__(256) k_gc_cost_final(const double* __restrict__ part, int n_chunks, const int* __restrict__ m, double* rec) {
  gc_final_body(part, n_chunks, rec);
  if (threadIdx.x == 0) { rec[GC_SUMS] = (double)*m; rec[GC_SUMS + 1] = 0.0; rec[GC_SUMS + 2] = 0.0; }
}

// ---- 4. the batch round (mi355ndt_gicp_batch_align, ndt_host_gicp_batch.hpp) -------------------------------------------
// One round serves every slot that waits for an evaluation: one table in device memory, first the slots asking for a matching pass, then
// the slots asking for a cost (at 64 slots the table is 20 KB, too large for kernel arguments).  A workgroup of 256 belongs to exactly one
// slot, found from the entries' first chunks (ascending: a slot's last, partial chunk is followed by the next slot's first chunk in the same
// grid), and runs the single-pair body on that slot's chunk.  Each slot keeps its own idx / maha / part / match counter and its own tree;
// k_gc_cost_final_batch, one workgroup per entry of the table, writes rec[slot][GC_REC] into mapped host memory: for a cost the sums and the
// m the host learned from the slot's matching pass, for a matching pass m alone -- and it clears the counter, which nothing reads until the
// slot's next matching pass adds to it (an integer atomic per wave, as in k_gc_match; no float atomics anywhere).
struct GcSlot {
  const float* src; const double* c1;              // the slot's cloud: rows [3][spitch], covariances [9][spitch]
  int* idx; double* maha; int* m; double* part;    // the slot's own correspondences, match counter and chunk partials
  double* rec;                                     // the slot's record in mapped host memory (the device's view)
  unsigned spitch; int n, chunk0, n_chunks;        // chunk0: the slot's first workgroup in its kernel's grid
  int m_host, pad;                                 // cost: the matches of the slot's last matching pass
  union { GcMatch match; GcCost cost; };
};

// the entry whose chunks hold workgroup `wg`: the last one with chunk0 <= wg (every entry has at least one chunk)
__device__ __forceinline__ const GcSlot& gc_slot_of(const GcSlot* __restrict__ tab, int n, int wg) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].chunk0 <= wg) lo = mid; else hi = mid - 1;
  }
  return tab[lo];
}

__global__ void __launch_bounds__(256) k_gc_match_batch(const GcSlot* __restrict__ tab, int n_entries, KfiView tgt, const double* __restrict__ c2) {
  const GcSlot& e = gc_slot_of(tab, n_entries, (int)blockIdx.x);
  gc_match_body(e.src, e.spitch, e.n, tgt, e.match, e.c1, c2, e.idx, e.maha, e.m, (int)blockIdx.x - e.chunk0);
}

__global__ void __launch_bounds__(GC_CHUNK) k_gc_cost_batch(const GcSlot* __restrict__ tab, int n_entries, const float* __restrict__ tgt, size_t tpitch) {
  const GcSlot& e = gc_slot_of(tab, n_entries, (int)blockIdx.x);
  gc_cost_body(e.src, e.spitch, e.n, tgt, tpitch, e.idx, e.maha, e.cost, e.part, (int)blockIdx.x - e.chunk0);
}

// entries 0 .. n_match - 1 asked for a matching pass, the rest for a cost
__global__ void __launch_bounds__(256) k_gc_cost_final_batch(const GcSlot* __restrict__ tab, int n_match) {
  const GcSlot& e = tab[blockIdx.x];
  const bool cost = (int)blockIdx.x >= n_match;
  if (cost) gc_final_body(e.part, e.n_chunks, e.rec);
  if (threadIdx.x == 0) {
    if (cost) {
      e.rec[GC_SUMS] = (double)e.m_host;
    } else {
      for (int k = 0; k < GC_SUMS; k++) e.rec[k] = 0.0;
      e.rec[GC_SUMS] = (double)*e.m;
      *e.m = 0;
    }
    e.rec[GC_SUMS + 1] = 0.0; e.rec[GC_SUMS + 2] = 0.0;
  }
}

// the source moved by the final transformation (pcl::transformPointCloud, the PCL 1.8 scalar form): x, y, z records of 12 B
__global__ void __launch_bounds__(256) k_gc_move(const float* __restrict__ src, size_t spitch, int n, GcCost a, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float px = src[i], py = src[spitch + i], pz = src[2 * spitch + i];
#pragma unroll
  for (int r = 0; r < 3; r++) out[3 * (size_t)i + r] = ((a.Tx[0 * 4 + r] * px + a.Tx[1 * 4 + r] * py) + a.Tx[2 * 4 + r] * pz) + a.Tx[3 * 4 + r];
}
