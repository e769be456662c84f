// ndt_sweep_exists.hpp -- THE table of the instantiations of k_sweep / k_sweep_pca_kd / k_align_async.  The three row lists below are the only place
// an instantiation is named; the predicates, the explicit instantiations of the three translation units, their `extern template` declarations
// and the host's run-time lookup (ndt_host_sweep.hpp: sweep_kernel, kd_kernel, launch_async) are all expansions of the rows: a kernel is added
// or removed by editing one row.  Nothing of HIP is compiled from this file unless a HIP translation unit expands a row into a kernel's name: it
// also compiles, with g++, into tests/cpp/*.cpp, which print the predicates as tables for tests/test_sweep_entries_cpu.py and friends.
#pragma once

// The columns:
//   PCA   false = ndt_omp, true = ndt_pca.  ndt_pca + KDTREE (K = 27) has the literal kernel k_sweep_pca_kd instead of a k_sweep row
//   K     cells probed: 1 / 7 / 26 / 27 (neighbor_K)
//   IT    64-point tiles per work item: 8 = batch-mode items (and the one-launch align, which has no other); 1 / 2 = latency mode's fine items,
//         DIRECT1 / DIRECT7 alone.  k_sweep's FINE tag is no column: it is IT != SWEEP_IT_BATCH
//   ORD   0 / 1 = the two f32 sum orders; 2 = the tolerance arithmetic, DIRECT1 / DIRECT7 alone (fast_served).  Always a literal 0 / 1 / 2: the
//         translation unit a kernel is compiled in is chosen by pasting this token (NDT_ROW_IN_TU_*)
//   PM    0 = SE(3); 1 = the Euler model (MI355NDT_OPT_POSE_MODEL = 1); 2 = PCL's class, the radius search and the f64 evaluation
//         (MI355NDT_OPT_NDT_CLASS = 1: the one row)
//   GATE  the gated probe stage of MI355NDT_OPT_GROUND_CLASS = 1 / 2, DIRECT searches (class 3 runs the ungated rows)
//   LEAN  k_align_async alone: the lean item body at three waves per SIMD, exact ndt_omp / DIRECT7 (ndt_sweep_waves.hpp; launch_async picks it
//         when the launch's AsyncLaunch::lean says so)
constexpr int SWEEP_IT_BATCH = 8;

// k_sweep: R(PCA, K, IT, ORD, PM, GATE)
#define NDT_SWEEP_ROWS(R)                                                                                                                       \
  R(false, 1, 8, 0, 0, false) R(true, 1, 8, 0, 0, false) R(false, 7, 8, 0, 0, false) R(true, 7, 8, 0, 0, false) /* batch items, exact */      \
  R(false, 26, 8, 0, 0, false) R(true, 26, 8, 0, 0, false) R(false, 27, 8, 0, 0, false)                                                        \
  R(false, 1, 8, 1, 0, false) R(true, 1, 8, 1, 0, false) R(false, 7, 8, 1, 0, false) R(true, 7, 8, 1, 0, false)                                \
  R(false, 26, 8, 1, 0, false) R(true, 26, 8, 1, 0, false) R(false, 27, 8, 1, 0, false)                                                        \
  R(false, 1, 8, 2, 0, false) R(true, 1, 8, 2, 0, false) R(false, 7, 8, 2, 0, false) R(true, 7, 8, 2, 0, false) /* batch items, tolerance */  \
  R(false, 1, 1, 0, 0, false) R(true, 1, 1, 0, 0, false) R(false, 1, 2, 0, 0, false) R(true, 1, 2, 0, 0, false) /* fine items */              \
  R(false, 7, 1, 0, 0, false) R(true, 7, 1, 0, 0, false) R(false, 7, 2, 0, 0, false) R(true, 7, 2, 0, 0, false)                                \
  R(false, 1, 1, 1, 0, false) R(true, 1, 1, 1, 0, false) R(false, 1, 2, 1, 0, false) R(true, 1, 2, 1, 0, false)                                \
  R(false, 7, 1, 1, 0, false) R(true, 7, 1, 1, 0, false) R(false, 7, 2, 1, 0, false) R(true, 7, 2, 1, 0, false)                                \
  R(false, 1, 1, 2, 0, false) R(true, 1, 1, 2, 0, false) R(false, 1, 2, 2, 0, false) R(true, 1, 2, 2, 0, false)                                \
  R(false, 7, 1, 2, 0, false) R(true, 7, 1, 2, 0, false) R(false, 7, 2, 2, 0, false) R(true, 7, 2, 2, 0, false)                                \
  R(false, 1, 8, 0, 1, false) R(false, 7, 8, 0, 1, false) R(false, 26, 8, 0, 1, false) R(false, 27, 8, 0, 1, false) /* the Euler model */     \
  R(false, 1, 8, 1, 1, false) R(false, 7, 8, 1, 1, false) R(false, 26, 8, 1, 1, false) R(false, 27, 8, 1, 1, false)                            \
  R(false, 27, 8, 0, 2, false)                                                                                    /* PCL's class */           \
  R(false, 1, 8, 0, 0, true) R(false, 7, 8, 0, 0, true) R(false, 26, 8, 0, 0, true)                               /* the gated sweep */       \
  R(false, 1, 8, 1, 0, true) R(false, 7, 8, 1, 0, true) R(false, 26, 8, 1, 0, true)
// k_sweep_pca_kd: R(ORD)
#define NDT_KD_ROWS(R) R(0) R(1)
// k_align_async: R(PCA, K, ORD, LEAN) -- every batch-mode SE(3) row of k_sweep, plus the lean bodies
#define NDT_ALIGN_ROWS(R)                                                                                                \
  R(false, 1, 0, false) R(true, 1, 0, false) R(false, 7, 0, false) R(true, 7, 0, false)                                  \
  R(false, 26, 0, false) R(true, 26, 0, false) R(false, 27, 0, false)                                                    \
  R(false, 1, 1, false) R(true, 1, 1, false) R(false, 7, 1, false) R(true, 7, 1, false)                                  \
  R(false, 26, 1, false) R(true, 26, 1, false) R(false, 27, 1, false)                                                    \
  R(false, 1, 2, false) R(true, 1, 2, false) R(false, 7, 2, false) R(true, 7, 2, false)                                  \
  R(false, 7, 0, true) R(false, 7, 1, true)

// ---- the predicates: a tag exists when it is a row ---------------------------------------------------------------------------------------------
struct SweepTag { bool pca; int K, it, ord, pm; bool gate; };
struct AlignTag { bool pca; int K, ord; bool lean; };
constexpr bool same(const SweepTag& a, const SweepTag& b) { return a.pca == b.pca && a.K == b.K && a.it == b.it && a.ord == b.ord && a.pm == b.pm && a.gate == b.gate; }
constexpr bool same(const AlignTag& a, const AlignTag& b) { return a.pca == b.pca && a.K == b.K && a.ord == b.ord && a.lean == b.lean; }
#define NDT_OR_SWEEP_ROW(PCA, K, IT, ORD, PM, GATE) || same(t, SweepTag{PCA, K, IT, ORD, PM, GATE})
#define NDT_OR_ALIGN_ROW(PCA, K, ORD, LEAN) || same(t, AlignTag{PCA, K, ORD, LEAN})
constexpr bool sweep_exists(const SweepTag& t) { return false NDT_SWEEP_ROWS(NDT_OR_SWEEP_ROW); }
constexpr bool align_exists(const AlignTag& t) { return false NDT_ALIGN_ROWS(NDT_OR_ALIGN_ROW); }
// ... and by family, as their callers ask: the SE(3) sweeps, the Euler model's, the gated ones, the lean one-launch align
constexpr bool sweep_exists(bool pca, int K, int ord, int it) { return sweep_exists(SweepTag{pca, K, it, ord, 0, false}); }
constexpr bool euler_sweep_exists(int K, int ord) { return sweep_exists(SweepTag{false, K, SWEEP_IT_BATCH, ord, 1, false}); }
constexpr bool ground_sweep_exists(int K, int ord) { return sweep_exists(SweepTag{false, K, SWEEP_IT_BATCH, ord, 0, true}); }
constexpr bool lean_exists(bool pca, int K, int ord) { return align_exists(AlignTag{pca, K, ord, true}); }

// ---- a row as a kernel's name, as an explicit instantiation or an `extern template` declaration (HIP translation units only) -------------------
#define NDT_SWEEP_TAG(PCA, K, IT, ORD, PM, GATE) k_sweep<PCA, K, IT, (IT != SWEEP_IT_BATCH), ORD, PM, GATE>
#define NDT_KD_TAG(ORD) k_sweep_pca_kd<ORD>
#define NDT_ALIGN_TAG(PCA, K, ORD, LEAN) k_align_async<PCA, K, ORD, LEAN>
// the kernels' parameter lists (ndt_sweep.hpp, ndt_sweep_kd.hpp, ndt_async.hpp)
#define NDT_SWEEP_ARGS_T (const float*, size_t, const PairState*, const GridDesc*, const BitWord*, const VoxelRec*, double*, int, const int*, SweepCtl*, SweepCtl*, \
                          SweepConst, const float*, const int*)
#define NDT_KD_ARGS_T (const float*, size_t, const PairState*, const GridDesc*, const BitWord*, const VoxelRec*, const float*, const int*, double*, int, const int*, \
                       SweepCtl*, SweepCtl*, SweepConst)
#define NDT_CTX_T const float*, size_t, PairState*, const GridDesc*, const BitWord*, const VoxelRec*, double*, const int*, unsigned*, const float*
#define NDT_ASYNC_ARGS_T (const AsyncTab*, int, int*, int, AsyncCtl*, SweepConst, unsigned long long*, double, double, int, int, unsigned, unsigned, int, NDT_CTX_T, NDT_CTX_T, NDT_CTX_T, NDT_CTX_T)
// The library is three translation units that compile side by side, split by ORD: mi355_ndt.hip instantiates the ORD = 0 rows where its host side
// names them and declares the others `extern template`; mi355_ndt_ord1.hip defines the ORD = 1 rows, mi355_ndt_fast.hip the ORD = 2 rows.  A unit
// says `#define NDT_TU ORD1 / FAST / ELSEWHERE` and `#define NDT_TU_X template` (or `extern template`), then expands NDT_KERNELS_OF_TU: the rows
// whose NDT_ROW_IN_TU_<unit>_<ORD> is 1.  Kernels only: no device function crosses the units.
#define NDT_ROW_IN_TU_ORD1_0 0
#define NDT_ROW_IN_TU_ORD1_1 1
#define NDT_ROW_IN_TU_ORD1_2 0
#define NDT_ROW_IN_TU_FAST_0 0
#define NDT_ROW_IN_TU_FAST_1 0
#define NDT_ROW_IN_TU_FAST_2 1
#define NDT_ROW_IN_TU_ELSEWHERE_0 0
#define NDT_ROW_IN_TU_ELSEWHERE_1 1
#define NDT_ROW_IN_TU_ELSEWHERE_2 1
#define NDT_KEEP_0(...)
#define NDT_KEEP_1(...) __VA_ARGS__
#define NDT_PASTE(a, b) a##b
#define NDT_KEEP(yes) NDT_PASTE(NDT_KEEP_, yes)
#define NDT_IF_ROW_IN_TU_(TU, ORD) NDT_KEEP(NDT_ROW_IN_TU_##TU##_##ORD)
#define NDT_IF_ROW_IN_TU(TU, ORD) NDT_IF_ROW_IN_TU_(TU, ORD)
#define NDT_SWEEP_ROW_OF_TU(PCA, K, IT, ORD, PM, GATE) NDT_IF_ROW_IN_TU(NDT_TU, ORD)(NDT_TU_X __global__ void NDT_SWEEP_TAG(PCA, K, IT, ORD, PM, GATE) NDT_SWEEP_ARGS_T;)
#define NDT_KD_ROW_OF_TU(ORD) NDT_IF_ROW_IN_TU(NDT_TU, ORD)(NDT_TU_X __global__ void NDT_KD_TAG(ORD) NDT_KD_ARGS_T;)
#define NDT_ALIGN_ROW_OF_TU(PCA, K, ORD, LEAN) NDT_IF_ROW_IN_TU(NDT_TU, ORD)(NDT_TU_X __global__ void NDT_ALIGN_TAG(PCA, K, ORD, LEAN) NDT_ASYNC_ARGS_T;)
#define NDT_KERNELS_OF_TU NDT_SWEEP_ROWS(NDT_SWEEP_ROW_OF_TU) NDT_KD_ROWS(NDT_KD_ROW_OF_TU) NDT_ALIGN_ROWS(NDT_ALIGN_ROW_OF_TU)
