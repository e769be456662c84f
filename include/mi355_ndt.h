/*
 * mi355_ndt.h -- C-ABI of the MI355X-native NDT scan-matching engine (libmi355ndt.so).
 *
 * Drop-in boundary for the one hot path of BurryChen/lv_slam: the pcl::Registration-style
 * setInputTarget / setInputSource / align surface implemented by
 *   pclomp::NormalDistributionsTransform  (include/ndt_omp/ndt_omp.h, ndt_omp_impl2.hpp)
 *   pclpca::NormalDistributionsTransform  (include/ndt_pca/ndt_pca.h,  ndt_pca_impl2.hpp)
 * and their VoxelGridCovariance target grids, as called from
 *   src/lidar_odometry/scan_matching_odom_nodelet.cpp:109-119,197,220-226,243  and
 *   include/global_graph/loop_detector.hpp:219,249-262.
 * Everything behind these entry points runs as hand-written HIP kernels on gfx950; there is
 * no CPU fallback: every call fails with MI355NDT_ERR_NO_DEVICE / MI355NDT_ERR_HIP when no GPU
 * is usable.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary; every call returns an int status.
 *   - 4x4 transforms are float[16] COLUMN-MAJOR (Eigen::Matrix4f's native layout):
 *     M(r,c) = m[c*4+r].
 *   - host point clouds are arrays of records whose first three floats are x,y,z, `stride_bytes`
 *     apart (16 for pcl::PointXYZ, 32 for pcl::PointXYZI / PointXYZRGBL).  The engine copies
 *     x,y,z out during the call; caller memory is never referenced afterwards.
 *   - a handle is bound to one HIP device and one stream and is NOT thread-safe (the reference
 *     object is driven by one thread at a time, scan_matching_odom_nodelet.cpp:56;
 *     global_graph_nodelet.cpp:672); distinct handles are independent.
 */
#ifndef MI355_NDT_H_
#define MI355_NDT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355NDT_OK               0
#define MI355NDT_ERR_BAD_HANDLE  (-1)
#define MI355NDT_ERR_BAD_ARG     (-2)
#define MI355NDT_ERR_HIP         (-3)  /* a HIP runtime call failed; see mi355ndt_last_error() */
#define MI355NDT_ERR_GRID        (-4)  /* target grid unusable: reference int32 guard
                                          (voxel_grid_covariance_omp_impl.hpp:75-84) or engine cell cap */
#define MI355NDT_ERR_NO_DEVICE   (-5)
#define MI355NDT_ERR_UNSUPPORTED (-6)  /* a surface or configuration MI355NDT_OPT_POSE_MODEL = 1, MI355NDT_OPT_NDT_CLASS = 1 or a non-zero MI355NDT_OPT_GROUND_CLASS does not serve (mi355ndt_last_error says which) */
/* Positive: a warning that rides in mi355ndt_result.status, never a return code.  Set only under MI355NDT_OPT_ARITH = 1: the registration is of a kind the
 * tolerance arithmetic is not meant for -- fewer than MI355NDT_TOLERANCE_MIN_HITS (point, voxel) hits at the final pose (the Hessian of a handful of points:
 * ~1e-7 per f32 term times its condition number is no tolerance-level perturbation any more) or a run that stopped at the iteration cap (an oscillating run
 * amplifies any rounding difference).  The result stands; a caller that needs the default arithmetic's robustness re-runs that pair with the option off (the
 * pcl adaptor and the python mirror do so by themselves). */
#define MI355NDT_WARN_TOLERANCE_ARITH 1
#define MI355NDT_TOLERANCE_MIN_HITS   4096
#define MI355NDT_ERR_STATE       (-7)  /* align/derivatives before target+source were set */

/* pclomp::NeighborSearchMethod, include/ndt_omp/ndt_omp.h:51-56 (same enum order) */
enum mi355ndt_neighbor { MI355NDT_KDTREE = 0, MI355NDT_DIRECT26 = 1, MI355NDT_DIRECT7 = 2, MI355NDT_DIRECT1 = 3 };
/* which reference class is emulated */
enum mi355ndt_variant { MI355NDT_VARIANT_OMP = 0 /* pclomp:: */, MI355NDT_VARIANT_PCA = 1 /* pclpca:: */ };

typedef struct mi355ndt_params {
  float  resolution;              /* setResolution            ndt_omp.h:126-136; ctor default 1.0f (ndt_omp_impl2.hpp:56) */
  double step_size;               /* setStepSize              ndt_omp.h:163;     default 0.1  (impl2:57) */
  double outlier_ratio;           /* setOulierRatio [sic]     ndt_omp.h:181;     default 0.55 (impl2:58) */
  double trans_epsilon;           /* setTransformationEpsilon (pcl::Registration); default 0.1 (impl2:78) */
  int    max_iterations;          /* setMaximumIterations     (pcl::Registration); default 35  (impl2:79) */
  int    neighbor_mode;           /* setNeighborhoodSearchMethod ndt_omp.h:186;  default DIRECT7 (impl2:81) */
  int    variant;                 /* 0 = ndt_omp, 1 = ndt_pca (integer voxel weight, ndt_pca_impl2.hpp:294-296) */
  int    min_points_per_voxel;    /* voxel_grid_covariance_omp.h:204 (6) */
  double min_covar_eigvalue_mult; /* voxel_grid_covariance_omp.h:205 (0.01) */
} mi355ndt_params;

typedef struct mi355ndt_result {
  float     final_colmajor[16];   /* getFinalTransformation()          (final_transformation_, impl2:900) */
  double    trans_probability;    /* getTransformationProbability()    (impl2:187) */
  double    score;                /* score of the last derivative sweep */
  int       iterations;           /* getFinalNumIteration()            (nr_iterations_) */
  int       converged;            /* hasConverged()                    (converged_) */
  int       sweeps;               /* computeDerivatives passes (1 + steps taken); live More-Thuente case: the count the
                                     reference makes -- repeated evaluations of an unchanged pose are reused, not re-run */
  int       status;               /* per-pair status: MI355NDT_OK, MI355NDT_ERR_GRID, or MI355NDT_WARN_TOLERANCE_ARITH (> 0: a result, with a caveat) */
  long long hits_last;            /* (point,voxel) evaluations in the last sweep */
} mi355ndt_result;

/* one searchable voxel as the sweep sees it (parity hook for VoxelGridCovariance::Leaf,
 * voxel_grid_covariance_omp.h:92-187) */
typedef struct mi355ndt_voxel {
  int32_t idx;        /* linear cell index (voxel_grid_covariance_omp_impl.hpp:223) */
  int32_t n;          /* nr_points; -1 = eigen / inverse failure (impl:339,363) -> never hit */
  double  mean[3];    /* mean_ */
  float   icov[9];    /* float(icov_), row-major (ndt_omp_impl2.hpp:576) */
  int32_t weight;     /* ndt_pca (int)dimension_2d_ (voxel_grid_covariance_pca.h:222-226); 1 for ndt_omp */
} mi355ndt_voxel;

typedef struct mi355ndt_profile {
  double    sweep_ms;        /* sum of derivative-sweep kernel durations (HIP events on the engine's stream) */
  long long sweep_launches;
  double    sweep_alg_bytes; /* algorithmic bytes of those launches: sum over active pairs of N*(12+4K) + 64*hits */
  long long sweep_hits;      /* (point,voxel) evaluations in those launches */
  long long sweep_points;    /* source points swept in those launches */
  double    build_ms;        /* sum of target-build durations (all voxelisation kernels + sort) */
  long long build_launches;  /* number of batch builds */
  double    build_alg_bytes; /* algorithmic bytes of the builds (DESIGN.md B_build) */
  double    update_ms;       /* sum of Newton-update kernel durations */
  long long update_launches;
  long long async_fallbacks; /* one-launch aligns that gave up (a wave's ticket never came within its poll budget) and were re-run by the
                                round-based path: same results, never an error */
  long long stream_launches; /* stream mode: persistent launches (one per submitted batch + flushes) */
  long long stream_carried;  /* stream mode: pairs handed over from one launch to the next (stragglers that finished under a later batch) */
  long long stream_redone;   /* stream mode: batches re-run synchronously (build plan exceeded, or a launch gave up) */
  long long cloud_uploads;   /* host clouds staged and sent over PCIe (set_target / set_source / batch_set_* / calculate_score / prefilter / batch_prefilter / map_cloud: its non-empty keyframes / window_keyframe: its non-empty scans / keyframe_add), counted always */
  long long cloud_upload_bytes;
  long long cloud_transfers;  /* host-to-device transfers those clouds travelled in (mi355ndt_batch_set_clouds / stream_submit_host send up to eight clouds per transfer) */
  long long cloud_promotions; /* mi355ndt_promote_source_to_target calls (device-to-device instead of an upload) */
  long long stream_reserved_slots; /* stream mode: workgroup slots the persistent launches leave to the next batch's build (the effective MI355NDT_OPT_STREAM_RESERVE; 0 = the build runs between the launches) */
  long long stream_launch_slots;   /* stream mode: workgroups of one persistent launch (CUs x workgroups per CU - the reserved slots).  Both: of the last launch that
                                      started a batch; before the first launch, what mi355ndt_stream_begin sized the session for (two workgroups per CU in the exact
                                      arithmetic -- a launch that takes the three-wave body, MI355NDT_OPT_SWEEP_WAVES, reports its own 768-slot geometry) */
  long long score_only_sweeps;     /* sweeps of the one-launch align that evaluated the score alone (MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP) */
  long long async_waves_per_simd;  /* the last persistent launch (one-launch align or stream launch; 0: none yet): waves per SIMD its kernel is built for
                                      (2; 3 = the lean exact DIRECT7 body, MI355NDT_OPT_SWEEP_WAVES; 3 / 4 in the tolerance arithmetic) ... */
  long long async_launch_slots;    /* ... and the workgroups it was launched with (CUs x waves per SIMD - the stream's reserved slots); not cleared by a reset */
} mi355ndt_profile;

typedef struct mi355ndt_handle mi355ndt_handle;

const char* mi355ndt_version(void);
int mi355ndt_device_count(void);                       /* number of usable HIP devices (0 on a CPU-only box) */
/* NUMA node of the host CPUs closest to `device` (-1 = unknown).  Host clouds are staged by CPU threads: on a two-socket host
 * a staging thread that reads the clouds across the socket link runs at half the rate, so keep the threads that own the
 * clouds (and call set_source / set_target) on this node; the engine's own staging threads pin themselves to it. */
int mi355ndt_host_numa_node(int device);

/* ctor defaults of NormalDistributionsTransform() (ndt_omp_impl2.hpp:53-83) */
int mi355ndt_default_params(mi355ndt_params* p);

/* replaces: `pclomp::NormalDistributionsTransform<PS,PT> reg;` (scan_matching_odom_nodelet.cpp:328,
 * registrations.cpp:78).  `params` may be NULL (defaults). */
int mi355ndt_create(const mi355ndt_params* params, int device, mi355ndt_handle** out);
int mi355ndt_destroy(mi355ndt_handle* h);

/* replaces the setters of ndt_omp.h:109-203.  A change of variant / min points / eigenvalue multiplier re-voxelises the current targets.
 * A change of `resolution` does what setResolution does (ndt_omp.h:126-136: `if (input_) init();`): the target is re-voxelised only when a
 * SOURCE has been set (mi355ndt_set_source / a bound batch); without one the resident grid keeps its leaf size until the next
 * mi355ndt_set_target, while the Gauss constants of the next align already use the new value (ndt_omp_impl2.hpp:93-100) -- the reference's
 * behaviour, quirk included.  Deviation: with KDTREE or the live More-Thuente configuration (radius searches over the grid) the target is
 * re-voxelised at once in either case. */
int mi355ndt_set_params(mi355ndt_handle* h, const mi355ndt_params* params);
int mi355ndt_get_params(const mi355ndt_handle* h, mi355ndt_params* out);

/* bind the engine to a caller-owned hipStream_t (NULL = the engine's own stream) */
int mi355ndt_set_stream(mi355ndt_handle* h, void* hip_stream);
const char* mi355ndt_last_error(const mi355ndt_handle* h);

/* ---- single registration: the pcl::Registration surface (pair slot 0) --------------------------- */

/* replaces setInputTarget(cloud) -> init() -> VoxelGridCovariance::filter(true)
 * (ndt_omp.h:116-121, 270-277; voxel_grid_covariance_omp_impl.hpp:48-370) */
int mi355ndt_set_target(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes);
/* replaces pcl::Registration::setInputSource(cloud) */
int mi355ndt_set_source(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes);
/* The cloud last handed over as SOURCE becomes the target (device-to-device copy + init()), without crossing PCIe again: the nodelet's keyframe switch
 * `key = filtered; reg_s2k.setInputTarget(key);` (scan_matching_odom_nodelet.cpp:240-243) right after `filtered` was aligned as the source.  Same result as
 * mi355ndt_set_target on the same cloud.  MI355NDT_ERR_STATE without a source (single-registration surface only). */
int mi355ndt_promote_source_to_target(mi355ndt_handle* h);
/* replaces align(output, guess) -> computeTransformation(output, guess) (ndt_omp_impl2.hpp:87-188) */
int mi355ndt_align(mi355ndt_handle* h, const float guess_colmajor[16], mi355ndt_result* out);
/* the `output` cloud of align(): source transformed by the final pose (f32, PCL 1.8 scalar form).
 * Writes x,y,z into records `stride_bytes` apart. */
int mi355ndt_get_aligned(mi355ndt_handle* h, void* out_pts, size_t stride_bytes);

/* pcl::Registration::transformation_ / previous_transformation_ as the last align() left them: float(exp(delta_p)) of the
 * last Newton step (ndt_omp_impl2.hpp:163; what getLastIncrementalTransformation() returns) and of the step before it
 * (impl2:134); both Identity when no step was taken.  Column-major 4x4; either pointer may be NULL.  `pair` = batch slot
 * (0 for the single-registration surface). */
int mi355ndt_get_incremental(mi355ndt_handle* h, int pair, float transformation_colmajor[16], float previous_colmajor[16]);

/* replaces pcl::Registration::getFitnessScore(max_range) as called by the loop-closure path
 * (include/global_graph/loop_detector.hpp:249-262; identical recipe in-tree:
 * src/global_graph/information_matrix_calculator.cpp:53-87): source moved by the final pose of the last align()
 * (identity before any align), exact nearest target point per source point, mean of the SQUARED distances that are
 * <= max_range (squared distance vs max_range, as the reference compares them); DBL_MAX when nothing is in range.
 * Works for any target cloud, also one whose voxel grid could not be built (status MI355NDT_ERR_GRID: exhaustive search).
 * It is mi355ndt_batch_fitness_scores on the one pair the handle holds: the first call after a target build adds an index of the target's
 * occupied cells (16 B per 64 grid cells + 4 B per target point of device memory), later calls only search. */
int mi355ndt_get_fitness_score(mi355ndt_handle* h, double max_range, double* score, long long* n_inliers);
/* same with an explicit transform (column-major 4x4) */
int mi355ndt_fitness_score_T(mi355ndt_handle* h, const float T_colmajor[16], double max_range, double* score, long long* n_inliers);

/* replaces calculateScore(cloud) (ndt_omp.h:232, ndt_omp_impl2.hpp:1006-1040; ndt_pca.h:244, ndt_pca_impl2.hpp:1013-1047): the negative
 * log-likelihood of an ALREADY TRANSFORMED cloud against the target grid, all in f64: per point the radiusSearch(point, resolution)
 * neighbourhood over the f32 leaf centroids (no nr_points re-check, voxel_grid_covariance_omp.h:505-534), per neighbour
 * (-d1 * exp(-d2 * x'^T icov x' / 2) - d3) / neighbourhood.size(), summed and divided by cloud.size().  d1, d2, d3 are the members
 * gauss_d1_/d2_/d3_ as the reference holds them when the call is made: the constructor's values (resolution 1.0, outlier ratio 0.55,
 * impl2:70-76) until the first align(), after that those of the last align()'s parameters (impl2:93-100).  No caller inside lv_slam.
 * `pts`: host records, x,y,z first, `stride_bytes` apart (typically the output cloud of align()). */
int mi355ndt_calculate_score(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes, double* score);

/* replaces the two static convertTransform helpers (ndt_omp.h:209-228): x = [x, y, z, roll, pitch, yaw] (f64) ->
 * Translation3f * AngleAxisf(roll, X) * AngleAxisf(pitch, Y) * AngleAxisf(yaw, Z) as a 4x4 f32 matrix, column-major -- what
 * Eigen::Affine3f::matrix() holds; evaluated in f32 the way Eigen 3.3 does (AngleAxis::toRotationMatrix, then the two 3x3 products).
 * Plain host arithmetic, no device needed. */
int mi355ndt_convert_transform(const double x[6], float out_colmajor[16]);

/* Engine options that are no parameter of the reference classes. */
enum mi355ndt_option {
  /* Evaluation order of the three-term f32 sums inside updateDerivatives (ndt_omp_impl2.hpp:581, 594-613: 4-wide Eigen inner
   * products whose fourth term is a structural zero).  The reference leaves that order to Eigen 3.3 and the SSE level it is
   * built for (CMakeLists.txt:6,11); it cannot be observed without the reference's libraries.  0 (default): (t0 + t1) + t2,
   * Eigen's scalar redux = the order every committed parity fixture was made with.  1: (t0 + t2) + t1, the lane pairing of Eigen 3.3's SSE
   * predux<Packet4f>.  Same cost; lets a maintainer who pins the reference on a real build (tools/pin_reference/) select the
   * order that build shows.  Poses differ in their last bits for about half of all pairs. */
  MI355NDT_OPT_F32_SUM_ORDER = 1,
  /* 1 (default): a batch align runs as ONE persistent launch in which every pair goes through its own Newton loop to its own end, as
   * every align() of the reference does (ndt_omp_impl2.hpp:131-183); 0: lockstep rounds of (update, sweep) launches over the pairs
   * still iterating.  Same results bit for bit (a pair's sums never depend on what runs beside it); the environment variable
   * MI355NDT_ASYNC=0 sets the default to 0 for engines created afterwards.  The one launch is used when the batch offers more work items
   * than the GPU has resident waves (smaller batches are faster in rounds); 2 = use it for every batch size (testing).  The latency mode and the live More-Thuente configuration
   * always take the round-based path. */
  MI355NDT_OPT_ASYNC_ALIGN = 2,
  /* Test hook, default -1 (off).  n >= 0: inside a one-launch align the wave that claims position n of ring 0 gives up exactly as a wave whose
   * ticket never came within its poll budget does: the launch ends early and mi355ndt_batch_align re-runs the batch through the round-based path
   * (mi355ndt_profile.async_fallbacks counts it).  Lets the test-suite exercise the fallback, which a healthy device never takes. */
  MI355NDT_OPT_DEBUG_ASYNC_ABORT = 3,
  /* Stream mode (mi355ndt_stream_*): a launch hands its last `value` unfinished pairs over to the next launch instead of iterating them alone
   * on an otherwise idle GPU.  -1 (default): as many as it takes to keep every resident wave busy (resident waves / work items per sweep);
   * 0: never (every launch runs its own pairs to the end: pipelining of the host side only).  No result bit depends on it. */
  MI355NDT_OPT_STREAM_THRESHOLD = 4,
  /* Stream mode, read by mi355ndt_stream_begin: the persistent launches leave `value` workgroup slots free (rounded down to a multiple of 8)
   * and the NEXT batch's target build runs on a stream of its own beside the launch instead of between two launches -- the build streams
   * through HBM, the launch saturates the vector ALUs.  Needs >= 3 contexts (a context is rebuilt one launch earlier, so its pairs are carried
   * through one launch less).  -1 (default): the environment variable MI355NDT_STREAM_RESERVE, else for DIRECT1 128 with clouds of up to 98,304 points and 96 beyond (launches that
   * wait for their point stream leave the vector ALUs to the build: +5-10 %), for DIRECT7 with batches of up to 768 x 65,536 target points 64 (ndt_omp; 96 of 768 slots where the launch runs
   * the three-wave body, MI355NDT_OPT_SWEEP_WAVES) / 32 (ndt_pca)
   * (the launch pays for the slots in full, the whole build disappears under it: +4-6 % at 271 pairs, +22 % at 64) and 0 = off for every other search.  No result bit depends on it. */
  MI355NDT_OPT_STREAM_RESERVE = 5,
  /* Test hook, default 0xFF (off).  Bit x clear: the workgroups of a one-launch align that serve ring x leave at once, as if XCD x held no
   * workgroup of this launch (another engine's launch filling it).  The launch must still finish every pair -- waiting waves serve the
   * published positions of other rings (ndt_async.hpp) -- with the same bits; mask 0 is refused. */
  MI355NDT_OPT_DEBUG_ASYNC_RINGS = 6,
  /* Arithmetic of the derivative sweep.  0 (default): every f32 / f64 operation of updateDerivatives (ndt_omp_impl2.hpp:566-619) as the CPU
   * restatement of the reference performs it, one rounding per operation, 43 f64 sums per lane -- results equal the CPU restatement's bit for bit.
   * 1: tolerance arithmetic, held to north_star's SE(3) tolerance (trans < 1e-4 m, rot < 1e-5 rad against the reference arithmetic) instead:
   * fused multiply-adds, the hardware exp2, a symmetric inverse covariance (21 symmetric + 9 point-Hessian sums instead of 36), f32 sums per
   * work item (512 points) widened to f64 from there on, leaf sums of the target build as a tree instead of in input order.  The point
   * transform and the voxel lookup are untouched (same leaves for the same pose).  Served for DIRECT1 / DIRECT7 with the dead More-Thuente
   * loop (every configuration lv_slam ships); other configurations ignore the option.  Measured cost in accuracy: BASELINE.md 5a. */
  MI355NDT_OPT_ARITH = 7,
  /* 1 (default): in the one-launch align, a pair's last derivative sweep -- the one whose convergence test (ndt_omp_impl2.hpp:175-179) is decided
   * when the step is scheduled, because it reads only the iteration count and the step length -- evaluates the score alone: its gradient and
   * Hessian are never read.  0: every sweep evaluates all 43 sums.  Same results bit for bit; mi355ndt_profile.score_only_sweeps counts the
   * score-only sweeps.  The environment variable MI355NDT_SCORE_ONLY_LAST_SWEEP sets the default for engines created afterwards.  Not changed
   * in stream mode. */
  MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP = 8,
  /* Cell size, in millimetres, of the spatial index mi355ndt_keyframe_fitness_scores builds over a searched keyframe (default 100).  The cell is
   * doubled until the keyframe's lattice has at most min(2^21, 64 x points) cells; a keyframe that does not get there within six doublings (a
   * stray point at 1e12 m) is searched exhaustively.  The search is exact for any cell: no result bit depends on the option, only the time.
   * Indexes that exist keep the cell they were built with. */
  MI355NDT_OPT_KF_FITNESS_CELL_MM = 9,
  /* Cell size, in millimetres, of the spatial index mi355ndt_prefilter_outliers builds over the prefilter result in every call (default 100,
   * the keyframe option's default until the timing tool's sweep has been run on a GPU: DESIGN.md 8), doubled by the keyframe option's rule.
   * The search is exact for any cell: no result bit depends on the option, only the time. */
  MI355NDT_OPT_OUTLIER_CELL_MM = 10,
  /* Raw clouds per group of mi355ndt_batch_prefilter (0, the default: as many as keep the engine's scratch under its 2 GiB budget, 4096 at the
   * most).  No result word depends on the option, only the time and the scratch; it exists so that a test can force several groups. */
  MI355NDT_OPT_PREFILTER_GROUP = 11,
  /* Which implementation of pclomp::NormalDistributionsTransform the aligns restate.  0 (default): include/ndt_omp/ndt_omp_impl2.hpp, the
   * Lie-algebra variant lv_slam compiles -- every result word as without the option.  1: include/ndt_omp/ndt_omp_impl.hpp, the Euler-angle NDT
   * of upstream ndt_omp and of PCL, which a host gets by changing the include line of src/ndt_omp/ndt_omp.cpp: the pose vector is
   * p = [x y z roll pitch yaw], started from the f32 translation and f32 rotation().eulerAngles(0, 1, 2) of the guess (a guess with negative
   * roll starts in the chart near roll = pi, as the reference does) and updated by p += delta_p; the point Jacobian and Hessian come from the
   * tables j_ang / h_ang applied to the ORIGINAL point; the pose matrix and the incremental transformations are convertTransform in f32.
   * Served under 1: mi355ndt_batch_align, mi355ndt_align, mi355ndt_derivatives (p read as [t; roll pitch yaw]), all four neighbour searches, both
   * f32 sum orders, always through the lockstep (update, sweep) rounds.  MI355NDT_OPT_ARITH is ignored (the exact arithmetic runs, no warning
   * status).  Refused with MI355NDT_ERR_UNSUPPORTED and a message, nothing changed: variant = PCA, the live More-Thuente configuration
   * (step_size <= trans_epsilon / 2), mi355ndt_sequence_run*, mi355ndt_stream_begin, mi355ndt_compute_hessian, mi355ndt_derivatives_T.  Setting
   * the option while a stream is open: MI355NDT_ERR_STATE; any other value: MI355NDT_ERR_BAD_ARG.  PCL's own f64 NormalDistributionsTransform
   * (registration_method = NDT) is not this option: it is MI355NDT_OPT_NDT_CLASS. */
  MI355NDT_OPT_POSE_MODEL = 12,
  /* Which class the aligns restate.  0 (default): pclomp::NormalDistributionsTransform -- every result word as without the option.  1:
   * pcl::NormalDistributionsTransform<PointXYZI, PointXYZI>, PCL's own class, which select_registration_method (src/global_graph/registrations.cpp)
   * hands out for registration_method = NDT and for every name it does not know.  It is the Euler-angle pose model (as MI355NDT_OPT_POSE_MODEL = 1:
   * the same pose vector, start, step, convertTransform in f32 and convergence rule) with PCL's evaluation: one neighbourhood,
   * radiusSearch(moved point, resolution) over the leaf centroids, and updateDerivatives in f64 from end to end -- the f32 moved point widened
   * minus the leaf's f64 mean, the leaf's f64 inverse covariance, the f64 j_ang / h_ang rows applied to the original point, exp in f64.
   * Under 1 neighbor_mode, MI355NDT_OPT_POSE_MODEL and MI355NDT_OPT_ARITH are not consulted (no warning status), and no result word depends on
   * MI355NDT_OPT_F32_SUM_ORDER: the evaluation has no three-term f32 sum, and the point transform and the radius test are written in one order.
   * Served under 1: mi355ndt_batch_align, mi355ndt_align, mi355ndt_derivatives (p read as [t; roll pitch yaw]), mi355ndt_get_fitness_score,
   * mi355ndt_batch_fitness_scores, host clouds and keyframe ids as sources and targets; an align always goes through the lockstep (update, sweep)
   * rounds.  Refused with MI355NDT_ERR_UNSUPPORTED and a message, nothing changed: variant = PCA, the live More-Thuente configuration
   * (step_size <= trans_epsilon / 2), mi355ndt_sequence_run*, mi355ndt_stream_begin, mi355ndt_compute_hessian, mi355ndt_derivatives_T.  Setting
   * the option while a stream is open: MI355NDT_ERR_STATE; any other value: MI355NDT_ERR_BAD_ARG.  A target that is resident without centroids
   * or f64 inverse covariances is rebuilt by the next align.  PCL's single-threaded GeneralizedIterativeClosestPoint (registration_method = GICP)
   * stays unserved. */
  MI355NDT_OPT_NDT_CLASS = 13,
  /* Waves per SIMD of the exact (MI355NDT_OPT_ARITH = 0) ndt_omp / DIRECT7 item body in the one-launch align and the stream's launches.  2: the
   * body with the mid-evaluation record prefetch and two-tile probe groups (245 VGPRs).  3: the lean body (168 VGPRs, no prefetch, one tile
   * probed at a time), 768 instead of 512 workgroup slots.  0 (default): decided per launch on the host -- three waves where the records of
   * the pairs in flight stay L2-resident, by an estimate from the leaf size and the points per target (ndt_host_sweep.hpp: async_lean), else
   * two.  Every other configuration (ndt_pca, DIRECT1, DIRECT26, KDTREE, the tolerance arithmetic, the lockstep rounds, the Euler model,
   * MI355NDT_OPT_NDT_CLASS = 1) ignores the option.  No result word depends on it: both bodies write the same rows bit for bit.  Setting it while
   * a stream is open: MI355NDT_ERR_STATE; any other value: MI355NDT_ERR_BAD_ARG.  The environment variable MI355NDT_SWEEP_WAVES sets the
   * default for engines created afterwards.  mi355ndt_profile.async_waves_per_simd reports what the last launch took. */
  MI355NDT_OPT_SWEEP_WAVES = 14,
  /* pclomp_ground::NormalDistributionsTransformGround (include/ndt_omp/ndt_ground.h, ndt_ground_impl.hpp), the class scan_matching_odom_nodelet
   * configures as ground_s2k.  0 (default): off -- pclomp's class, every result word as without the option.  1: flag_class 1, the value its
   * computeTransformation hard-codes: only points whose LAST neighbour (in the search's order) is a horizontal leaf (normal within 10 degrees of
   * z) add their sums, and rows and columns 0, 1, 5 of the Hessian and the gradient are zeroed, so only z, roll and pitch move.  2: flag_class 2:
   * vertical leaves (more than 80 degrees), rows and columns 2, 3, 4 zeroed.  3: flag_class 0: every point, nothing zeroed.  Under 1, 2 and 3
   * alike the reference evaluates every hit twice into the gradient and the Hessian and once into the score, so g and H are twice ndt_omp's over
   * the same hits, and its convergence test has no `nr_iterations_ &&` guard: an align can end after its first step.  The leaf's normal is the
   * eigenvector of the smallest eigenvalue of its un-inflated covariance; the angle is acos(|n_z|) * 180 / 3.1415926, compared strictly.
   * Served: mi355ndt_batch_align, mi355ndt_align, mi355ndt_derivatives (the doubled and masked sums), mi355ndt_calculate_score and the fitness
   * scores (unchanged), with variant = OMP, DIRECT1 / DIRECT7 / DIRECT26, both f32 sum orders, always through the lockstep (update, sweep) rounds;
   * MI355NDT_OPT_ARITH and latency mode are ignored.  Refused with MI355NDT_ERR_UNSUPPORTED and a message, nothing changed: variant = PCA, the
   * live More-Thuente configuration (its computeHessian is unmasked), KDTREE (the last neighbour of a radius search is FLANN's to order),
   * MI355NDT_OPT_POSE_MODEL = 1 or MI355NDT_OPT_NDT_CLASS = 1 beside a non-zero value, mi355ndt_sequence_run*, mi355ndt_stream_begin,
   * mi355ndt_compute_hessian, mi355ndt_derivatives_T.  Setting the option while a stream is open: MI355NDT_ERR_STATE; any other value:
   * MI355NDT_ERR_BAD_ARG.  A resident target that lacks the leaves' class codes is rebuilt by the next align under 1 or 2. */
  MI355NDT_OPT_GROUND_CLASS = 15
};
int mi355ndt_set_option(mi355ndt_handle* h, int option, int value);
int mi355ndt_get_option(const mi355ndt_handle* h, int option, int* value);

/* parity hooks ------------------------------------------------------------------------------------ */
/* one computeDerivatives sweep (ndt_omp_impl2.hpp:196-305) at tangent p = [upsilon; omega]:
 * points transformed by float(exp(p)), Jacobian from the same matrix (impl2:900-907).
 * H is 6x6 row-major and NOT symmetric. */
int mi355ndt_derivatives(mi355ndt_handle* h, const double p[6], double* score, double g[6], double H[36], long long* hits);
/* computeHessian + updateHessian (ndt_omp_impl2.hpp:622-714) at tangent p: the f64 Hessian-only pass over kd-tree
 * neighbourhoods that computeStepLengthMT runs after its More-Thuente loop iterated (impl2:999-1000; live only when
 * step_size <= transformation_epsilon/2).  Cloud moved by float(exp(p)).  H is 6x6 row-major. */
int mi355ndt_compute_hessian(mi355ndt_handle* h, const double p[6], double H[36]);
/* same sweep with an explicit point transform (column-major 4x4) and Jacobian rotation (row-major 3x3),
 * i.e. the first sweep of align() where the cloud is moved by the caller's guess (impl2:102-129) */
int mi355ndt_derivatives_T(mi355ndt_handle* h, const float T_colmajor[16], const float Rj_rowmajor[9],
                           double* score, double g[6], double H[36], long long* hits);
/* The partial rows the last sweep of every pair of the bound batch left on the device: per pair *rows_per_pair rows of 44 doubles (score, g[6],
 * H[36] row-major, hits) -- one row per work item of 512 source points in batch mode --, pair after pair, `capacity` doubles at the most
 * (MI355NDT_ERR_BAD_ARG when the rows need more; `out` may be NULL to ask for *rows_per_pair alone).  A row's bits depend on the pair, the pose
 * and the input order alone: never on the kernel, the launch geometry or the wave that ran the item.  A score-only last sweep
 * (MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP) writes a row's score and hits and leaves the sweep before it in the other 42 words.
 * MI355NDT_ERR_STATE before the first align of the batch, and in stream mode. */
int mi355ndt_get_partial_rows(mi355ndt_handle* h, double* out, size_t capacity, int* rows_per_pair);
/* target grid of pair `pair`: bounds (min_b_, max_b_, div_b_) and searchable voxels in ascending idx order */
int mi355ndt_get_grid(mi355ndt_handle* h, int pair, int min_b[3], int max_b[3], int div_b[3], int* n_voxels);
int mi355ndt_get_voxels(mi355ndt_handle* h, int pair, mi355ndt_voxel* out, size_t capacity);
/* One target's part of one buffer of the target build, raw, as the build's kernels left it (the stage tests read every kernel's output with it).
 * Read-only: waits for the handle's stream, copies to the host, launches nothing.  Valid only directly after a synchronous
 * mi355ndt_batch_build_targets: MI355NDT_ERR_STATE in stream mode and when the grids are not valid; MI355NDT_ERR_BAD_ARG for an unknown `which`,
 * for a buffer that build did not make (centroids, f64 inverse covariances, kd weights, tolerance records, sorted points) and when
 * capacity_bytes is too small.  *bytes receives the size; `out` may be NULL to ask for it alone.  Per-leaf buffers hold n_voxels entries. */
enum mi355ndt_build_buffer {
  MI355NDT_BUILD_MINMAX = 0,         /* 6 unsigned: the encoded extremes min x y z, max x y z (0 = no finite point) */
  MI355NDT_BUILD_GRIDDESC = 1,       /* the grid descriptor: int min_b[3] max_b[3] div_b[3] mul1 mul2, float leaf inv_leaf, int ncells nwords status n_voxels, unsigned word_off rec_off */
  MI355NDT_BUILD_WORDS = 2,          /* nwords x {uint64 bits, uint32 prefix, uint32 pad} */
  MI355NDT_BUILD_KEYS = 3,           /* pitch unsigned: the sorted cell keys */
  MI355NDT_BUILD_IDS = 4,            /* pitch unsigned: the point index of every sorted position */
  MI355NDT_BUILD_HEAD_CNT = 5,       /* n_slices unsigned */
  MI355NDT_BUILD_HEADS = 6,          /* n_slices x slice_cap unsigned (the first head_cnt of every slice are written) */
  MI355NDT_BUILD_SEG_START = 7,      /* n_voxels unsigned */
  MI355NDT_BUILD_SUMS = 8,           /* n_voxels x 9 double: S0 S1 S2 C00 C01 C02 C11 C12 C22 */
  MI355NDT_BUILD_CENT = 9,           /* n_voxels x 3 float */
  MI355NDT_BUILD_VOX_IDX = 10,       /* n_voxels int */
  MI355NDT_BUILD_VOX_N = 11,         /* n_voxels int (-1: dead) */
  MI355NDT_BUILD_ICOV64 = 12,        /* n_voxels x 9 double */
  MI355NDT_BUILD_KD_WEIGHT = 13,     /* n_voxels int */
  MI355NDT_BUILD_RECS_FAST = 14,     /* n_voxels x 64 bytes: float mh[3] ml[3] c[6] pad[3], int weight */
  MI355NDT_BUILD_SORTED_POINTS = 15, /* pitch x 4 float (MI355NDT_LEAF_SORTED engines only) */
  MI355NDT_BUILD_INFO = 16,          /* 2 unsigned, pair-independent: bitmap words of the batch, cells of its largest grid */
  MI355NDT_BUILD_GEOMETRY = 17       /* 5 uint64, pair-independent: pitch, records per pair, n_slices, slice_cap, key bits */
};
/* ... and the one buffer only a build under MI355NDT_OPT_GROUND_CLASS = 1 / 2 makes (MI355NDT_ERR_BAD_ARG after any other build), numbered on from
 * the table above: n_voxels unsigned char, the class of every leaf record -- 0 dead (not a neighbour), 1 normal within 10 degrees of the z axis,
 * 2 beyond 80 degrees, 3 neither. */
enum mi355ndt_build_buffer_ground {
  MI355NDT_BUILD_LEAF_CLASS = 18
};
int mi355ndt_get_build_buffer(mi355ndt_handle* h, int which, int pair, void* out, size_t capacity_bytes, size_t* bytes);

/* ---- batch: n independent (target, source, guess) triples on one GPU ---------------------------- */
/* (BASELINE.json configs 3-5; the single-registration calls above are the n = 1 case) */

int mi355ndt_batch_reserve(mi355ndt_handle* h, int n_pairs, size_t max_target_pts, size_t max_source_pts);
/* Host uploads into pair slot `pair` (same record convention as set_target / set_source).  Asynchronous: the call returns as
 * soon as x,y,z of the caller's records sit in one of the engine's pinned staging slots (caller memory is not referenced
 * afterwards); the PCIe transfer and the AoS -> SoA kernel run on the engine's copy stream while the next cloud is staged, and
 * the next build / align waits for them.  These two calls -- and only these -- may be issued from several threads at once for
 * DIFFERENT pair slots (staging is the CPU-bound part of a host-cloud batch). */
int mi355ndt_batch_set_target(mi355ndt_handle* h, int pair, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_batch_set_source(mi355ndt_handle* h, int pair, const void* pts, size_t n, size_t stride_bytes);
/* A whole batch of host clouds in one call: pairs first_pair .. first_pair + n - 1, one pointer and one point count per cloud
 * (`targets` or `sources` may be NULL to upload only the other side), records `stride_bytes` apart; n_threads staging threads
 * of the engine's own (<= 0: 8) share the pairs.  Same asynchrony as the per-cloud calls.  Every pair's arguments are checked before anything
 * is staged: a NULL pointer with a count, a stride below 12 or a count above what was reserved returns MI355NDT_ERR_BAD_ARG with the batch unchanged. */
int mi355ndt_batch_set_clouds(mi355ndt_handle* h, int first_pair, int n, const void* const* targets, const size_t* target_counts,
                              const void* const* sources, const size_t* source_counts, size_t stride_bytes, int n_threads);
/* zero-copy: use device-resident SoA buffers laid out [pair][3][pitch] (x row, y row, z row of `pitch`
 * floats each).  counts are HOST arrays of n_pairs ints.  The buffers must stay valid until replaced. */
int mi355ndt_batch_bind_device(mi355ndt_handle* h, int n_pairs,
                               const float* d_targets, const int* target_counts, size_t target_pitch,
                               const float* d_sources, const int* source_counts, size_t source_pitch);
/* voxelise every target (setInputTarget for all pairs); asynchronous on the engine's stream */
int mi355ndt_batch_build_targets(mi355ndt_handle* h);
/* align every pair; guesses = n_pairs x 16 floats column-major; out = n_pairs results. Synchronous. */
int mi355ndt_batch_align(mi355ndt_handle* h, const float* guesses_colmajor, mi355ndt_result* out);
int mi355ndt_batch_size(const mi355ndt_handle* h);
/* getFitnessScore(max_range) for every batch slot: source p moved by T[p], exact nearest target-p point per source point, mean of the
 * squared distances <= max_range; DBL_MAX and 0 inliers when nothing is in range or target p is empty.  T_colmajor = n_pairs x 16
 * floats column-major, or NULL = each pair's final pose of the last mi355ndt_batch_align (the identity before any align of the current
 * batch).  n_inliers may be NULL.  Synchronous.  scores[p] / n_inliers[p] are bit for bit what mi355ndt_fitness_score_T returns on a
 * one-pair engine holding pair p's clouds and T[p] (the same search: that call is the batch of one), also for a target without a grid
 * (MI355NDT_ERR_GRID: exhaustive search).  One exception: a pair with an EMPTY source (or target) scores DBL_MAX, 0 here, where the one-pair call refuses (MI355NDT_ERR_STATE).  Builds the
 * targets first if they are not built; MI355NDT_ERR_STATE in stream mode.  The loop detector's verification of K candidates against one
 * new keyframe (loop_detector.hpp:148-281) is one batch_align + one call of this (lv_slam_amd/loop_closure.py). */
int mi355ndt_batch_fitness_scores(mi355ndt_handle* h, const float* T_colmajor, double max_range, double* scores, long long* n_inliers);
/* Many start poses per pair scored in one call.  For item e: the score and the hit count that one computeDerivatives sweep (ndt_omp_impl2.hpp:196-305)
 * yields for pair pairs[e] of the bound batch with its source moved by the f32 matrix poses_colmajor[16 e .. 16 e + 15] -- the first sweep of an
 * align from that guess (impl2:102-129).  Gradient and Hessian are not evaluated.  scores[e] and hits[e] (hits may be NULL) are bit for bit what
 * mi355ndt_derivatives_T(T_e, any Rj) returns on a one-pair engine that holds the pair's two clouds with the same parameters and the same
 * MI355NDT_OPT_F32_SUM_ORDER, latency mode off; a row's bits depend on the pair, the pose and the input order alone.  Items may name pairs in any
 * order, a pair many times or not at all; a pair whose target has no searchable voxel scores 0.0 with 0 hits.  Host clouds and keyframe ids in
 * the slots; the grids are built first if they are not.  Synchronous: one copy of the call's tables in, two launches, one wait.  The call has a
 * pose table, a row buffer and a landing block of its own: the pair states, the results of the last mi355ndt_batch_align, the partial rows
 * (mi355ndt_get_partial_rows) and the incremental transforms (mi355ndt_get_incremental) are what they were.  n_items == 0 launches nothing.
 * Served: variant OMP and PCA with DIRECT1 / DIRECT7 / DIRECT26, OMP with KDTREE, both f32 sum orders.
 * Refused before anything is enqueued, nothing changed, with a mi355ndt_last_error text: MI355NDT_ERR_STATE in stream mode;
 * MI355NDT_ERR_UNSUPPORTED for ndt_pca + KDTREE (order-dependent weights, a kernel of its own), MI355NDT_OPT_POSE_MODEL = 1,
 * MI355NDT_OPT_NDT_CLASS = 1, a non-zero MI355NDT_OPT_GROUND_CLASS, and MI355NDT_OPT_ARITH = 1 (its grids are tree-summed and its records are
 * another layout: serving it is a later change); MI355NDT_ERR_BAD_ARG for n_items above MI355NDT_SCORE_POSES_MAX_ITEMS, a pair index outside
 * the batch and a pose with a non-finite entry.  This is not a call of the reference: lv_slam_amd/loop_closure.py (verify_candidates_search)
 * uses it to pick the start of a loop check from a lattice of poses around the guess. */
#define MI355NDT_SCORE_POSES_MAX_ITEMS 65536
int mi355ndt_batch_score_poses(mi355ndt_handle* h, int n_items, const int* pairs, const float* poses_colmajor, double* scores, long long* hits);
/* Pose records of the last mi355ndt_batch_align for the multi-GPU gather, written on the device into a caller-owned DEVICE
 * buffer of `capacity` 96-byte records {float final[16] column-major; float score; int32 iterations; int32 converged;
 * int32 pair_id; int32 pad[4]}: record k describes batch slot k and carries pair_id = id_base + k * id_stride (round-robin
 * sharding: base = rank, stride = world size); records k >= batch size carry pair_id = -1.  The buffer can go straight into
 * an RCCL all-gather: no host hop.  Returns after the records are complete (the engine's stream is synchronised). */
int mi355ndt_batch_pose_records(mi355ndt_handle* h, int id_base, int id_stride, void* d_records, size_t capacity);

/* ---- stream mode: batches arrive one after the other and overlap on the GPU --------------------------------------------------- */
/* The reference's odometry node consumes a continuous stream of frames (scan_matching_odom_nodelet.cpp:144-183: one cloud_callback per
 * scan); BASELINE config 3 streams batches of independent scan pairs through one GPU.  mi355ndt_batch_align is synchronous: build, ONE
 * persistent launch, results on the host, and only then the next batch -- the last pairs of a batch iterate alone on an idle GPU (the
 * tail), and the host's own work between two batches is dead time.  In stream mode the engine keeps `n_contexts` batches resident:
 *   submit(k)  enqueues batch k's target build, its persistent launch and the result copies, and returns at once;
 *   a launch ends as soon as its unfinished pairs can no longer keep the GPU busy; those pairs are SUSPENDED and become the first tickets of
 *              the next launch, where they finish under batch k+1's bulk (a pair runs the same code on the same operands whichever launch
 *              serves it: results are bit-identical to mi355ndt_batch_align's);
 *   collect(k) blocks until every pair of batch k is finalised -- normally a launch or two after its own; if nothing newer has been
 *              submitted it flushes the stragglers itself.
 * Batch k's context is recycled by submit(k + n_contexts), so at most n_contexts batches may be uncollected.  A pair is carried through at
 * most n_contexts - 2 further launches (one with two contexts): a batch is complete one launch before its context is recycled, so that the
 * host can collect it and enqueue the next build while a launch is still running.  Four contexts suit workloads whose launches end in long
 * tails (BASELINE config 5), three or four anything else.
 * Inputs are device-resident SoA buffers as in mi355ndt_batch_bind_device (zero-copy); batch k's buffers must stay valid and unchanged
 * until collect(k) has returned.  Parameters and options are those of the handle at mi355ndt_stream_begin; the handle's single-registration
 * and batch calls are unavailable (MI355NDT_ERR_STATE) between begin and end.  Served for every configuration the one-launch align
 * serves (DIRECT1/7/26 and ndt_omp KDTREE, dead More-Thuente loop: everything lv_slam ships); others are processed synchronously
 * inside submit. */
int mi355ndt_stream_begin(mi355ndt_handle* h, int n_contexts /* 2..4 */, int max_pairs, size_t max_target_pts, size_t max_source_pts);
int mi355ndt_stream_submit(mi355ndt_handle* h, int n_pairs, const float* d_targets, const int* target_counts, size_t target_pitch,
                           const float* d_sources, const int* source_counts, size_t source_pitch, const float* guesses_colmajor,
                           long long* batch_id);
/* The same for HOST clouds -- what the node has (scan_matching_odom_nodelet.cpp:144-183: pcl::PointCloud records arriving one callback at a time): arrays of
 * n_pairs pointers to the targets' / sources' records (x, y, z as the first three floats of every `stride_bytes`-long record, as mi355ndt_set_target takes
 * them) and their point counts.  The clouds are staged by `n_threads` threads of the engine (0 = 8) into the batch context's pinned slots, cross PCIe and land in
 * the context's own device buffers while the launches of earlier batches run; returns as soon as the caller's memory is no longer needed.  Counts must not
 * exceed what mi355ndt_stream_begin was told.  Results: word for word those of mi355ndt_batch_set_clouds + batch_build_targets + batch_align. */
int mi355ndt_stream_submit_host(mi355ndt_handle* h, int n_pairs, const void* const* targets, const size_t* target_counts, const void* const* sources,
                                const size_t* source_counts, size_t stride_bytes, const float* guesses_colmajor, int n_threads, long long* batch_id);
int mi355ndt_stream_collect(mi355ndt_handle* h, long long batch_id, mi355ndt_result* out);
/* Pose records for the multi-GPU gather (the 96-byte layout of mi355ndt_batch_pose_records) of the NEXT batch submitted: `d_records` is a
 * caller-owned DEVICE buffer of `capacity` records (>= that batch's pairs); record b is written by the device -- by the very wave that
 * finalises pair b, inside the persistent launch: no packing kernel, no host hop -- with pair_id = id_base + b * id_stride, the other rows
 * carry pair_id = -1.  Complete when mi355ndt_stream_collect of that batch has returned; the buffer can then go straight into an RCCL
 * all-gather.  NULL = no records for the next batch (the default). */
int mi355ndt_stream_pose_records(mi355ndt_handle* h, void* d_records, size_t capacity, int id_base, int id_stride);
/* Pose records (the 96-byte layout of mi355ndt_batch_pose_records) of a COLLECTED batch, packed on the host from its results into
 * `records` (host memory, `capacity` records; rows >= n carry pair_id = -1).  In stream mode the GPU is busy with the next batch's launch when
 * a batch is collected -- a packing kernel would wait for that launch -- so the 26 KB of a 271-pair batch are packed here and go to the device
 * with the caller's own copy.  Plain host arithmetic, no device needed. */
int mi355ndt_pack_pose_records(const mi355ndt_result* results, int n, int id_base, int id_stride, void* records, size_t capacity);
int mi355ndt_stream_end(mi355ndt_handle* h);      /* collects nothing: outstanding batches are dropped after the device has drained */

/* ---- latency mode: one frame at a time, as the live nodelet runs ---------------------------------------- */
/* Opt-in fine-grained derivative sweep for SMALL batches (a single registration above all): work items of 128 points dealt over
 * every wave of the GPU instead of 512-point items (a 65,536-point pair then offers 512 items to the 2,048 resident waves instead
 * of 128) and no work-queue atomics.  The per-pair f64 summation tree is this mode's own (fixed, deterministic, independent of
 * the batch a pair is in), NOT the batch mode's: a sweep agrees with the batch mode's to the rounding of the f64 sums (~1e-16
 * relative, inside the 1e-11 sweep bar); poses are normally bit-identical, but that is not promised across the two modes.
 * Applies to DIRECT1 / DIRECT7 with step_size > transformation_epsilon / 2 (everything lv_slam ships); other configurations
 * keep the batch kernels.  Default: off. */
int mi355ndt_set_latency_mode(mi355ndt_handle* h, int on);

/* keyframe policy of ScanMatchingOdomNodelet (scan_matching_odom_nodelet.cpp:67-76; launch/dlo_kitti.launch:51-53) */
typedef struct mi355ndt_seq_params {
  double keyframe_delta_trans;   /* [m]   default 5.0 in code, 10 in the KITTI launch file */
  double keyframe_delta_angle;   /* [rad] default 0.17 */
  double keyframe_delta_time;    /* [s]   default 1.0  */
} mi355ndt_seq_params;

typedef struct mi355ndt_seq_frame {
  double odom_colmajor[16];      /* odom_velo = key_pose * tf_s2k (:234): pose of the scan in the first keyframe's frame, 4x4 f64 column-major */
  float  tf_s2k_colmajor[16];    /* getFinalTransformation() of the scan-to-keyframe align (:222, :226) */
  double trans_probability;      /* getTransformationProbability() of that align */
  double dx, da, dt;             /* the three keyframe-test quantities (:237-239) */
  int    key_id;                 /* the keyframe this scan was matched against */
  int    new_keyframe;           /* 1: the test fired and this scan became the keyframe (:240-247) */
  int    iterations, converged;  /* of the (last) align of this scan */
  int    aligns;                 /* 2 for frame 1 (:223-227), 1 otherwise, 0 for frame 0 */
  int    pad;
} mi355ndt_seq_frame;

typedef struct mi355ndt_seq_stats {
  double    upload_ms;           /* host clouds -> HBM (staging + PCIe + AoS->SoA), host clock */
  double    build_ms;            /* voxel grids of all frames (one batched build), HIP events */
  double    track_ms;            /* frame 1 .. n-1: every align + the policy, HIP events; no host round trip inside */
  long long aligns;              /* n_frames (frame 1 twice, frame 0 never) */
  long long update_launches;     /* k_seq_update launches executed, incl. the pump's overshoot at the end */
} mi355ndt_seq_stats;

/* replaces n_frames calls of the nodelet's cloud_callback -> matching_s2k (scan_matching_odom_nodelet.cpp:144-183, 192-261):
 * the frames are uploaded, every frame's voxel grid is built (one batched build: every frame is a potential keyframe), and then
 * frame after frame is aligned against its keyframe with the guess, the keyframe test and the target switch decided ON THE DEVICE
 * at the tail of the Newton-update kernel -- the host pumps (update, sweep) launches without waiting for any result.  Uses the
 * handle's registration parameters (the nodelet's: resolution 1.0, DIRECT1, eps 0.01, 64 iterations, :109-119) and the
 * fine-grained sweep of mi355ndt_set_latency_mode.  `stamps` = header.stamp of every frame in seconds.  out_frames: n_frames
 * records; out_results (may be NULL): the engine-level result of every frame's last align; stats (may be NULL).
 * The call CONSUMES the handle's batch state: the frames replace whatever batch / single registration was resident (target, source,
 * voxel grids, last align), and none is resident afterwards -- set_target / set_source again before the next align(), or use a
 * handle of its own for the drive. */
int mi355ndt_sequence_run(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                          const double* stamps, const mi355ndt_seq_params* policy,
                          mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results, mi355ndt_seq_stats* stats);

/* ---- prefilter: the step immediately upstream of the path ------------------------------------------- */
/* replaces PrefilteringNodelet::distance_filter + downsample (src/lidar_odometry/prefiltering_nodelet.cpp:137-181,
 * launch/dlo_kitti.launch:30-36): keep near < |p| < far, then pcl::VoxelGrid centroid down-sampling with leaf
 * `downsample_resolution` (<= 0: none), output ordered by ascending voxel index.  The result stays on the GPU
 * (mi355ndt_use_prefiltered) and is copied to out_pts (x,y,z records, may be NULL) when it fits out_capacity.
 * It is mi355ndt_prefilter_p (below) with these four parameters and the rest at their defaults -- no move, no
 * calibration, VOXELGRID --: one implementation, the same words. */
int mi355ndt_prefilter(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes,
                       int use_distance_filter, double distance_near, double distance_far, float downsample_resolution,
                       void* out_pts, size_t out_capacity, size_t out_stride_bytes, size_t* n_out);
/* install the last prefilter result as the registration source (role 1) or target (role 2) without a host round trip */
int mi355ndt_use_prefiltered(mi355ndt_handle* h, int role);

/* ---- prefilter of whole batches: raw scans straight into the batch slots ------------------------------- */
/* The nodelet's parameters.  With use_transform every raw point is first moved by T = transform_colmajor (4x4 f32, column-major), the
 * nodelet's base_link move (prefiltering_nodelet.cpp:100-115: pcl_ros::transformPointCloud, which casts the tf transform to float and calls
 * PCL 1.8.1's pcl::transformPointCloud(in, out, Eigen::Matrix4f)):  (float)(((T(a,0) x + T(a,1) y) + T(a,2) z) + T(a,3)),  every product and sum
 * a separately rounded f32 operation; a point with a non-finite coordinate is not moved and is dropped by the filter.  The rule is PCL's as
 * restated here, unpinned.
 * With use_angle_calibration (mi355ndt_prefilter_params_ex) every point is then turned by angle_calibration_rad about the normalised p x (0,0,1)
 * (vertical_angle_calibration, :183-220): in f64, Eigen 3.3's cross, normalize (a point on the z axis keeps a zero axis and is scaled by
 * cos), AngleAxisd::toRotationMatrix and 3x3 product restated operation for operation, no FMA, the result cast to f32; a point with a
 * non-finite coordinate is left as it is.  The gate and the centroids see the moved and calibrated points.
 * downsample_method = MI355NDT_DOWNSAMPLE_APPROX_VOXELGRID is pcl::ApproximateVoxelGrid (PCL 1.8.1 approximate_voxel_grid.hpp; the intensity: mi355ndt_prefilter_params_ex2):
 * inv = 1.0f / leaf; cell = (int)floor(coord * inv), the product f32; a history table of 512 entries indexed by
 * (ix * 7171 + iy * 3079 + iz * 4231) & 511, walked in input order; a point whose entry holds another cell flushes it -- f32 sum / (float)count
 * is appended to the output --; after the last point the non-empty entries are flushed in table order.  A cell can appear more than once and
 * the output can be as large as the input.  Non-finite points are dropped, gate or no gate.  A cloud with a kept point whose
 * |floor(coord * inv)| >= 2^31 is left un-down-sampled under the "leaf too small" rule below.  Both rules as restated in
 * tools/prefilter_options_ref.py, unpinned. */
enum { MI355NDT_DOWNSAMPLE_VOXELGRID = 0, MI355NDT_DOWNSAMPLE_APPROX_VOXELGRID = 1 };
typedef struct mi355ndt_prefilter_params {
  int    use_distance_filter;           /* 1 */
  int    extended;                      /* 0.  MI355NDT_PREFILTER_EXTENDED: this struct is the `base` of the mi355ndt_prefilter_params_ex below.  The
                                           word lies where the compiler's padding lay: size and offsets of this struct are what they were */
  double distance_near, distance_far;   /* 1.0, 100.0: the nodelet's in-code defaults (prefiltering_nodelet.cpp:83-85) */
  float  downsample_resolution;         /* 0.1; <= 0: no down-sampling */
  int    use_transform;                 /* 0 */
  float  transform_colmajor[16];        /* identity */
} mi355ndt_prefilter_params;
int mi355ndt_prefilter_params_default(mi355ndt_prefilter_params* p);

/* The nodelet's remaining parameters, behind the struct above: mi355ndt_prefilter_params keeps its 96 bytes, so a caller built against it
 * goes on working unchanged, and every function that takes a `const mi355ndt_prefilter_params*` (mi355ndt_batch_prefilter,
 * mi355ndt_sequence_run_raw, mi355ndt_sequence_run_raw_outliers, mi355ndt_prefilter_p) also takes `&ex.base` of this one: when
 * base.extended == MI355NDT_PREFILTER_EXTENDED the three fields behind `base` are read, with any other value they are not looked at and
 * the defaults hold (VOXELGRID, no calibration).  mi355ndt_prefilter_params_ex_default fills `base` as mi355ndt_prefilter_params_default
 * does, sets base.extended and the three defaults. */
#define MI355NDT_PREFILTER_EXTENDED 0x50467832   /* "PFx2" */
typedef struct mi355ndt_prefilter_params_ex {
  mi355ndt_prefilter_params base;       /* base.extended = MI355NDT_PREFILTER_EXTENDED */
  int    downsample_method;             /* MI355NDT_DOWNSAMPLE_VOXELGRID; base.downsample_resolution <= 0 is "NONE" whatever the method */
  int    use_angle_calibration;         /* 0 (prefiltering_nodelet.cpp:88) */
  double angle_calibration_rad;         /* 0.11 * M_PI / 180, the reference's constant (:190) */
} mi355ndt_prefilter_params_ex;
int mi355ndt_prefilter_params_ex_default(mi355ndt_prefilter_params_ex* p);

/* The fourth channel of pcl::PointXYZI, behind the two structs above in the same way: mi355ndt_prefilter_params keeps its 96 bytes and
 * mi355ndt_prefilter_params_ex its size and offsets, and every function that takes a `const mi355ndt_prefilter_params*` also takes
 * `&ex2.ex.base`.  With base.extended == MI355NDT_PREFILTER_EXTENDED2 the three fields of `ex` are read as under MI355NDT_PREFILTER_EXTENDED,
 * and intensity_offset_bytes >= 0 names an f32 in every input record -- the point's intensity -- that goes through the chain beside x, y, z:
 *   the base_link move leaves it alone, also for a point it does not move;
 *   use_angle_calibration ZEROES it: vertical_angle_calibration builds a fresh point and assigns x, y, z (prefiltering_nodelet.cpp:207-210), the
 *     PointXYZI constructor leaves intensity = 0, so with the calibration on every output intensity is +0.0f -- a quirk of the reference,
 *     reproduced;
 *   a point the gate drops takes its intensity with it; a kept point's non-finite intensity is kept and goes into the sums as f32 gives it;
 *   VOXELGRID: the f32 sum of the voxel's intensities in input order / (float)count (CentroidPoint<PointXYZI>, AccumulatorIntensity), what
 *     mi355ndt_window_keyframe does; APPROX_VOXELGRID: the history entry's fourth sum (downsample_all_data_), from zero, in input order,
 *     divided by (float)count at every flush; no down-sampling, or a leaf too small: the kept point's own;
 *   the outlier removals: a survivor keeps its own, the row is compacted with the points' and its tail zeroed.
 * x, y, z come out word for word as without it.  PCL 1.8.1's rules as restated in tools/prefilter_xyzi_ref.py, unpinned.
 * MI355NDT_ERR_BAD_ARG, before anything is staged: intensity_offset_bytes + 4 > stride_bytes, an offset below 12 (it would overlap x, y, z),
 * an offset that is no multiple of 4, reserved != 0.  intensity_offset_bytes = -1: no intensity, every word as under
 * MI355NDT_PREFILTER_EXTENDED. */
#define MI355NDT_PREFILTER_EXTENDED2 0x50467833   /* "PFx3" */
typedef struct mi355ndt_prefilter_params_ex2 {
  mi355ndt_prefilter_params_ex ex;      /* ex.base.extended = MI355NDT_PREFILTER_EXTENDED2 */
  int    intensity_offset_bytes;        /* -1: no intensity; >= 0: an f32 at that offset of every record */
  int    reserved;                      /* 0 */
} mi355ndt_prefilter_params_ex2;
int mi355ndt_prefilter_params_ex2_default(mi355ndt_prefilter_params_ex2* p);

/* mi355ndt_prefilter with the nodelet's whole parameter set (p: a mi355ndt_prefilter_params or the base of a mi355ndt_prefilter_params_ex;
 * NULL: the defaults): the base_link move, the calibration, the gate and the
 * down-sampling method of p, by the batch surface's kernels over this one cloud.  The result stays resident exactly as after
 * mi355ndt_prefilter -- mi355ndt_use_prefiltered and mi355ndt_prefilter_outliers follow unchanged --, and with the default method and no
 * calibration its words are mi355ndt_prefilter's.  A leaf too small for the cloud is no error: the kept points go out in input order and
 * mi355ndt_last_error says so.  MI355NDT_ERR_BAD_ARG for what mi355ndt_prefilter and mi355ndt_batch_prefilter refuse.
 * With an intensity (mi355ndt_prefilter_params_ex2) the resident result has a fourth row, and the intensity is written into out_pts at the
 * input's offset: out_stride_bytes must hold it, else MI355NDT_ERR_BAD_ARG.  mi355ndt_prefilter_outliers carries the row and writes it to its
 * out_pts likewise (the same condition on its out stride); mi355ndt_use_prefiltered hands x, y, z to the registration as ever. */
int mi355ndt_prefilter_p(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes, const mi355ndt_prefilter_params* p,
                         void* out_pts, size_t out_capacity, size_t out_stride_bytes, size_t* n_out);

/* Like mi355ndt_batch_set_clouds, but every cloud is RAW and goes through the prefilter (mi355ndt_prefilter's rules, bit for bit) on its way
 * into its slot: the clouds are staged into the engine's scratch, filtered there group by group -- every stage one launch for all clouds of a
 * group, one wait for the device per group, none per cloud -- and emitted into the slots' own rows, whose tails are zeroed as an upload leaves
 * them.  mi355ndt_batch_reserve comes first; its two sizes are capacities for the FILTERED clouds, a raw count may exceed them (each below
 * 2^30).  Either side may be NULL (with its counts); p == NULL: the defaults above.  target_counts_out / source_counts_out (may be NULL)
 * receive the filtered counts.  mi355ndt_batch_build_targets / mi355ndt_batch_align follow as after mi355ndt_batch_set_clouds.
 * A leaf too small for some cloud's extent is no error: that cloud goes in as its kept points, in input order, and mi355ndt_last_error names
 * the first such slot.  MI355NDT_ERR_STATE in stream mode.  MI355NDT_ERR_BAD_ARG, every argument checked before anything is staged and
 * the batch unchanged: device buffers bound, a NULL cloud with a count, a stride below 12, a NaN resolution, a NaN in the transform, an unknown
 * downsample_method, a non-finite angle_calibration_rad, slots outside the batch.  MI355NDT_ERR_BAD_ARG also for a filtered cloud that does not fit its slot: mi355ndt_last_error names the first such
 * slot, and every slot the call touched is recorded as empty.  The resident prefilter result, the keyframes and their indexes are left as
 * they were.  MI355NDT_OPT_PREFILTER_GROUP.
 * With an intensity (mi355ndt_prefilter_params_ex2) the filtered intensities go into a plane per side beside the slots' rows ([slot][pitch],
 * made by the first such call that touches the side, dropped by mi355ndt_batch_reserve), and every slot the call fills is marked as carrying
 * one.  Every other route that fills a slot -- mi355ndt_batch_set_*, mi355ndt_batch_set_clouds, the keyframe setters,
 * mi355ndt_batch_bind_device, this call without an intensity -- clears the mark; mi355ndt_batch_remove_outliers compacts the marked slots'
 * intensities with their points; the builds, the aligns, the fitness scores and the sequence run do not look at it.  A call that fails
 * leaves the marks of the slots it touched clear. */
int mi355ndt_batch_prefilter(mi355ndt_handle* h, int first_pair, int n,
                             const void* const* targets, const size_t* target_counts,
                             const void* const* sources, const size_t* source_counts, size_t stride_bytes,
                             const mi355ndt_prefilter_params* p,
                             size_t* target_counts_out, size_t* source_counts_out /* either may be NULL */);

/* the points a batch slot holds (role 1 = source, 2 = target) as x,y,z records, whatever route filled the slot; waits for pending uploads
 * and kernels.  out_pts == NULL: the count alone.  MI355NDT_ERR_BAD_ARG for a bad slot or role and for a capacity below the count;
 * MI355NDT_ERR_STATE in stream mode. */
int mi355ndt_batch_get_cloud(mi355ndt_handle* h, int pair, int role, void* out_pts, size_t out_capacity,
                             size_t out_stride_bytes, size_t* n_out);
/* ... and with the slot's intensity as an f32 at out_intensity_offset_bytes (>= 12, a multiple of 4, inside the record) of every record:
 * what the batch prefilter left there, zeros for a slot that carries none (mi355ndt_keyframe_get's rule). */
int mi355ndt_batch_get_cloud_i(mi355ndt_handle* h, int pair, int role, void* out_pts, size_t out_capacity,
                               size_t out_stride_bytes, int out_intensity_offset_bytes, size_t* n_out);

/* mi355ndt_sequence_run over RAW scans: the same call with the batch prefilter in front, no scan downloaded in between.  The batch is
 * reserved for the raw counts.  stats->upload_ms covers the staging of the raw scans, *prefilter_ms (may be NULL) the prefilter's kernels
 * (HIP events); filtered_counts (may be NULL): n_frames filtered counts.  A frame that is empty after the prefilter is MI355NDT_ERR_BAD_ARG. */
int mi355ndt_sequence_run_raw(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                              const double* stamps, const mi355ndt_prefilter_params* pf, const mi355ndt_seq_params* policy,
                              mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results, mi355ndt_seq_stats* stats,
                              size_t* filtered_counts /* may be NULL */, double* prefilter_ms /* may be NULL */);

/* replaces PrefilteringNodelet::outlier_removal (prefiltering_nodelet.cpp:128, 150-161), the nodelet's last stage, over the RESIDENT
 * prefilter result, in place: the survivors keep their order, the result's count and rows are updated, and mi355ndt_use_prefiltered
 * installs the filtered cloud.  (A cloud that needs only this stage goes through mi355ndt_prefilter first, distance filter off and
 * resolution <= 0.)  Searchable points are those with three finite coordinates; squared distances are f32, (dx*dx + dy*dy) + dz*dz.
 *   STATISTICAL (pcl::StatisticalOutlierRemoval, the nodelet's in-code default, :61-70): per point, the mean_k + 1 smallest squared
 *     distances over the searchable points, itself included; sorted ascending, the first dropped; dist = (float)(sum of
 *     (double)sqrtf(d2) in ascending order / mean_k).  A non-finite point, or any point of a cloud with fewer than mean_k + 1
 *     searchable points, has dist = 0 and is not valid.  f64, in index order over every dist (zeros included): sum, sq;
 *     mean = sum / n_valid; var = (sq - sum * sum / n_valid) / (n_valid - 1); threshold = mean + stddev_mul * sqrt(var).  A point is
 *     removed iff (double)dist > threshold: non-valid points survive, and with n_valid of 0 or 1 the threshold is NaN and all survive.
 *   RADIUS (pcl::RadiusOutlierRemoval): kept iff at least min_neighbors searchable points other than itself have d2 < (float)(radius *
 *     radius), strictly; coincident points count; non-finite points are removed.  NOTE: the reference never runs this branch -- it
 *     builds the filter and does not assign it (:71-78), so under its launch files, which all ask for RADIUS, nothing is removed.  A
 *     host that wants the reference's behaviour under those launch files must not call this function.
 * mean_distances (may be NULL): dist of the n_in input points, input order (zeros for RADIUS).  out_pts / out_capacity /
 * out_stride_bytes / n_out as in mi355ndt_prefilter.  stats (may be NULL): STATISTICAL only, zeros for RADIUS.  The rules are PCL 1.8's
 * and FLANN's as restated in tools/outlier_ref.py, unpinned.  MI355NDT_ERR_STATE when no prefilter result is resident
 * or in stream mode; MI355NDT_ERR_BAD_ARG with a mi355ndt_last_error text for an unknown method, mean_k outside 1..64, min_neighbors
 * outside 0..64, a NaN or negative radius, a NaN stddev_mul.  An empty resident cloud gives *n_out = 0.  Synchronous, two waits for
 * the device (dist comes back once: the index-order sums are the host's).  The batch, the grids, the keyframes and their indexes, the
 * map-cloud and window workspaces of the handle are left as they were.  MI355NDT_OPT_OUTLIER_CELL_MM. */
enum { MI355NDT_OUTLIER_STATISTICAL = 1, MI355NDT_OUTLIER_RADIUS = 2 };
typedef struct mi355ndt_outlier_params {
  int method; int mean_k; double stddev_mul;      /* STATISTICAL: 20, 1.0  (prefiltering_nodelet.cpp:63-64) */
  double radius; int min_neighbors;               /* RADIUS: 0.8, 2        (:72-73) */
} mi355ndt_outlier_params;
typedef struct mi355ndt_outlier_stats {           /* STATISTICAL only; zeros for RADIUS */
  long long n_in, n_valid; double mean, stddev, threshold;
} mi355ndt_outlier_stats;
int mi355ndt_outlier_params_default(mi355ndt_outlier_params* p);   /* method STATISTICAL and the five defaults above */
int mi355ndt_prefilter_outliers(mi355ndt_handle* h, const mi355ndt_outlier_params* p,
                                float* mean_distances /* may be NULL; n_in floats, input order */,
                                void* out_pts, size_t out_capacity, size_t out_stride_bytes,
                                size_t* n_out, mi355ndt_outlier_stats* stats /* may be NULL */);

/* PrefilteringNodelet::outlier_removal over the clouds that batch slots first_pair .. first_pair + n - 1 hold, in place, whatever route
 * filled them.  sides: bit 0 = sources, bit 1 = targets.  Rules and params: mi355ndt_prefilter_outliers', word for word per cloud -- the
 * NOTE on RADIUS included: the reference builds that filter and never runs it.  One launch chain serves all clouds of a group (groups are cut
 * as mi355ndt_batch_prefilter cuts them, MI355NDT_OPT_PREFILTER_GROUP), the f64 statistics are formed on the device in index order, and the
 * call waits for the device once per group: no dist[] crosses PCIe.  Per cloud: the survivors keep their order, the slot's rows behind the
 * new count are zero as an upload leaves them, the slot's count is updated (a touched target invalidates the resident grids), and
 * mi355ndt_batch_build_targets / mi355ndt_batch_align follow unchanged.  An empty slot stays empty and its stats are zeros; for RADIUS all
 * stats are zeros.  target_counts_out / source_counts_out (n each, either may be NULL) receive the counts of the sides asked for;
 * target_stats / source_stats (n each, either may be NULL) their statistics.  MI355NDT_ERR_STATE in stream mode.  MI355NDT_ERR_BAD_ARG,
 * every argument checked before anything is enqueued and every slot, count and grid left as it was: device buffers bound, sides outside
 * 1..3, slots outside the batch, a side that has never been given a cloud, and every parameter mi355ndt_prefilter_outliers refuses (the same
 * texts behind "batch_remove_outliers:").  The resident prefilter result and its index, the keyframes and their indexes, the map-cloud and
 * window workspaces are left as they were.  MI355NDT_OPT_OUTLIER_CELL_MM.  The rules are PCL 1.8's and FLANN's as restated in
 * tools/outlier_ref.py, unpinned. */
int mi355ndt_batch_remove_outliers(mi355ndt_handle* h, int first_pair, int n, int sides, const mi355ndt_outlier_params* p /* NULL: defaults */,
                                   size_t* target_counts_out, size_t* source_counts_out,          /* either may be NULL */
                                   mi355ndt_outlier_stats* target_stats, mi355ndt_outlier_stats* source_stats /* n each; either may be NULL */);

/* mi355ndt_sequence_run_raw with the nodelet's third stage behind the batch prefilter: outlier != NULL runs mi355ndt_batch_remove_outliers
 * over the frames' slots before the sequence (outlier == NULL: mi355ndt_sequence_run_raw itself).  filtered_counts are the counts after
 * both stages, *prefilter_ms covers both stages' kernels, and a frame that is empty after both stages is MI355NDT_ERR_BAD_ARG. */
int mi355ndt_sequence_run_raw_outliers(mi355ndt_handle* h, int n_frames, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                                       const double* stamps, const mi355ndt_prefilter_params* pf, const mi355ndt_outlier_params* outlier,
                                       const mi355ndt_seq_params* policy, mi355ndt_seq_frame* out_frames, mi355ndt_result* out_results,
                                       mi355ndt_seq_stats* stats, size_t* filtered_counts /* may be NULL */, double* prefilter_ms /* may be NULL */);

/* ---- map cloud: the global graph's map (MapCloudGenerator::generate) ------------------------------------ */
/* replaces MapCloudGenerator::generate(keyframes, resolution) (src/global_graph/map_cloud_generator.cpp:17-55), which
 * GlobalGraphNodelet::optimization_timer_callback (global_graph_nodelet.cpp:725-745) and save_map_service (:1036-1046) call
 * over every keyframe: keyframe k's clouds[k] (counts[k] records of stride_bytes, x,y,z f32 first) moved by poses[16k..16k+15]
 * (KeyFrameSnapshot::pose.matrix(), column-major f64; cast to f32 as the reference does), all points fed in keyframe order into
 * pcl::octree::OctreePointCloud(resolution), and the occupied voxel centres written to out_pts as x,y,z f32 records (may be
 * NULL) in the order getOccupiedVoxelCenters returns them.  The input order matters: the first finite point anchors the
 * octree's lattice.  *n_out always gets the count; if it exceeds out_capacity the call returns MI355NDT_ERR_BAD_ARG and
 * writes nothing.  n_keyframes == 0 (the reference returns nullptr) and clouds without a finite point give *n_out = 0.
 * MI355NDT_ERR_BAD_ARG also for resolution <= 0, NaN or infinite, 2^30 points or more in all, and for points that would
 * need an octree deeper than 21 levels (2^21 voxels per axis: 105 km at 0.05 m; mi355ndt_last_error says so).  Intensity is
 * not carried (the reference's centres carry 0).  Synchronous; MI355NDT_ERR_STATE in stream mode.  Uses buffers of its
 * own: the batch, grids, prefilter result and stream state of the handle are left as they were. */
int mi355ndt_map_cloud(mi355ndt_handle* h, int n_keyframes, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                       const double* poses, double resolution, void* out_pts, size_t out_capacity,
                       size_t out_stride_bytes, size_t* n_out);

/* ---- keyframes that stay on the device: window map, keyframe store, consumers by id ---------------------- */
/* replaces the window accumulation and down-sampling of GlobalGraphNodelet::cloud_callback (global_graph_nodelet.cpp:202-244):
 * scan 0 as it is (:206, :232 `w_cloud = *cloud`), scan k > 0 moved by rel_poses[16k..] = (w_odom.inverse() * odom_k).matrix(),
 * column-major f64, the way PCL 1.8's transformPointCloud<PointT, double> moves it (:241: x, y, z widened to f64, one rounding
 * to f32 per coordinate), appended in scan order (:242), then pcl::VoxelGrid(leaf) over the whole window (:214-218: centroids
 * of x, y, z and -- with intensity_offset_bytes >= 0, the byte offset of an f32 in every record -- of the intensity; f32 sums in
 * input order; output in ascending voxel index).  rel_poses of scan 0 is ignored (rel_poses may be NULL for one scan).  Points
 * with a non-finite coordinate are dropped.  leaf <= 0: no down-sampling, the finite points of the window in order; a leaf too
 * small for the window's extent (PCL's "Leaf size is too small") does the same and says so in mi355ndt_last_error.  The
 * result stays on the device as keyframe *id; *n_out gets its point count.  MI355NDT_ERR_BAD_ARG for n_scans <= 0, a NaN
 * leaf, 2^30 points or more in all.  MI355NDT_ERR_STATE in stream mode.  Uses buffers of its own: the batch, grids, prefilter
 * result and map-cloud workspace of the handle are left as they were. */
int mi355ndt_window_keyframe(mi355ndt_handle* h, int n_scans, const void* const* scans, const size_t* counts, size_t stride_bytes,
                             int intensity_offset_bytes /* < 0: no intensity */, const double* rel_poses, float leaf,
                             int* id, size_t* n_out);
/* The keyframe store.  A keyframe owns [3 or 4][pitch] f32 rows on the device (x, y, z, and the intensity when it carries
 * one; pitch = count rounded up to 64, the tail zeroed).  Ids count up from 0 and are never reused within a handle; an
 * unknown or released id is MI355NDT_ERR_BAD_ARG with a message.  mi355ndt_keyframe_add stores a host cloud as it is (no
 * filtering, non-finite points included).  mi355ndt_keyframe_get writes x, y, z (and, with out_intensity_offset_bytes >= 0,
 * the intensity, 0 for a keyframe without one) into records of out_stride_bytes; out_pts NULL: the count only; a count above
 * out_capacity is MI355NDT_ERR_BAD_ARG with *n set.  All are MI355NDT_ERR_STATE in stream mode and leave the rest of the
 * handle as it was; mi355ndt_destroy frees the keyframes that are left. */
int mi355ndt_keyframe_add(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes, int intensity_offset_bytes, int* id);
int mi355ndt_keyframe_get(mi355ndt_handle* h, int id, void* out_pts, size_t out_capacity, size_t out_stride_bytes,
                          int out_intensity_offset_bytes, size_t* n);
int mi355ndt_keyframe_release(mi355ndt_handle* h, int id);
int mi355ndt_keyframe_count(const mi355ndt_handle* h);
/* Resident scans.  The resident prefilter result (after mi355ndt_prefilter* / mi355ndt_prefilter_outliers), or the cloud a batch slot holds
 * (role 1 = source, 2 = target; with its intensity when the slot carries one), becomes a keyframe of 3 or 4 channels by a device-to-device
 * copy on the engine's stream into rows the keyframe owns: nothing in the store aliases a slot or the prefilter result, and the source is left
 * as it was.  Pending uploads and kernels into the source are ordered before the copy.  An empty cloud gives an empty keyframe.
 * MI355NDT_ERR_STATE in stream mode, and for mi355ndt_keyframe_from_prefiltered when no result is resident; MI355NDT_ERR_BAD_ARG for a bad slot
 * or role and for a side that has never been given a cloud. */
int mi355ndt_keyframe_from_prefiltered(mi355ndt_handle* h, int* id);
int mi355ndt_keyframe_from_slot(mi355ndt_handle* h, int pair, int role, int* id);
/* mi355ndt_window_keyframe over resident scans: scan k is keyframe ids[k] as it is stored -- the same rules, the same words as over the
 * same clouds given as host records, and nothing crosses PCIe on the way in (cloud_uploads does not move).  with_intensity != 0: a keyframe
 * of four channels; a scan stored with three contributes +0 for every point.  An id may appear more than once; a released or unknown id is
 * MI355NDT_ERR_BAD_ARG with the store's message.  The scans' keyframes are left as they were: the host releases them when the window has
 * closed. */
int mi355ndt_window_keyframe_ids(mi355ndt_handle* h, int n_scans, const int* ids, const double* rel_poses, float leaf,
                                 int with_intensity, int* id, size_t* n_out);
/* mi355ndt_map_cloud over resident keyframes: the same result, word for word, as mi355ndt_map_cloud over the same clouds,
 * with nothing crossing PCIe on the way in (cloud_uploads does not move).  A keyframe may appear more than once. */
int mi355ndt_map_cloud_keyframes(mi355ndt_handle* h, int n_keyframes, const int* ids, const double* poses, double resolution,
                                 void* out_pts, size_t out_capacity, size_t out_stride_bytes, size_t* n_out);
/* mi355ndt_batch_set_target / _source with a resident keyframe, device to device, after mi355ndt_batch_reserve (the keyframe
 * must fit the reserved points; the intensity is not carried).  Everything downstream is as after the host-cloud setters. */
int mi355ndt_batch_set_target_keyframe(mi355ndt_handle* h, int pair, int id);
int mi355ndt_batch_set_source_keyframe(mi355ndt_handle* h, int pair, int id);

/* ---- graph edges between resident keyframes: fitness scores and information matrices ------------------------ */
/* replaces InformationMatrixCalculator::calc_fitness_score(cloud1, cloud2, relpose, max_range)
 * (src/global_graph/information_matrix_calculator.cpp:53-87) for E graph edges at once, over resident keyframes -- the odometry edge of
 * every new keyframe (global_graph_nodelet.cpp:298) and every accepted loop (:697).  Per edge e: keyframe ids1[e] is the searched cloud
 * (the kd-tree side), keyframe ids2[e] is moved by relposes[16e..] (column-major f64, cast entry-wise to f32 as relpose.cast<float>()
 * does, applied in the PCL 1.8 scalar form); each moved point takes its exact nearest point of cloud1; scores[e] is the mean of the
 * SQUARED distances that are <= max_range (squared distance vs max_range, as the reference compares them), DBL_MAX with 0 inliers when
 * nothing is in range or either keyframe is empty.  Points with a non-finite coordinate take no part, on either side.  scores[e] and
 * n_inliers[e] (may be NULL) are word for word what mi355ndt_fitness_score_T returns on a one-pair engine with cloud1 as target, cloud2 as
 * source and the f32-cast pose as T.  A keyframe may appear in any number of edges and on either side; ids1[e] == ids2[e] is allowed.
 * The first call that searches a keyframe builds a spatial index over it unless the GICP surface has (a keyframe has one index, which both
 * surfaces search); it stays with the keyframe until it is released (at most 16 + 20 B per point beside the keyframe's own 12;
 * MI355NDT_OPT_KF_FITNESS_CELL_MM); later calls find it.  n_edges == 0 is MI355NDT_OK;
 * an unknown or released id is MI355NDT_ERR_BAD_ARG with a message and nothing is written; MI355NDT_ERR_STATE in stream mode.  Nothing
 * crosses PCIe on the way in (cloud_uploads does not move); synchronous, one wait for the device per call.  Uses buffers of its own: the
 * batch, grids, prefilter result, map-cloud and window workspaces of the handle are left as they were. */
int mi355ndt_keyframe_fitness_scores(mi355ndt_handle* h, int n_edges, const int* ids1, const int* ids2,
                                     const double* relposes /* 16 per edge, column-major f64 */, double max_range,
                                     double* scores, long long* n_inliers /* may be NULL */);

/* The weighting half of InformationMatrixCalculator::calc_information_matrix (information_matrix_calculator.cpp:27-51,
 * include/global_graph/information_matrix_calculator.hpp:40-44), as written, quirks included: the variance bounds are the stddev
 * bounds squared; weight = min + (max - min) * (1 - exp(-a x)) / (1 - exp(-a thresh)) with NO clamp (a DBL_MAX score gives a weight
 * slightly above max); the weight is stored in a float before every entry of the 3x3 block of Identity(6,6) is divided by it; with
 * use_const_inf_matrix the blocks are divided by the STDDEV, not the variance (:32-33), and the score is not read.  inf: 6x6, row-major
 * (the matrix is diagonal).  Plain host arithmetic: no handle, no device.
 * mi355ndt_inf_params_default gives the constructor's defaults (:11-20; fitness_score_thresh 0.5).  Note that the reference's other
 * initialiser, load() (information_matrix_calculator.hpp:32), defaults the threshold to 2.5. */
typedef struct mi355ndt_inf_params {
  int    use_const_inf_matrix;
  double const_stddev_x, const_stddev_q, var_gain_a, min_stddev_x, max_stddev_x, min_stddev_q, max_stddev_q, fitness_score_thresh;
} mi355ndt_inf_params;
void mi355ndt_inf_params_default(mi355ndt_inf_params* p);
int  mi355ndt_information_matrix(const mi355ndt_inf_params* p, double fitness_score, double inf[36]);

/* ---- GICP: pclomp::GeneralizedIterativeClosestPoint (registration_method = GICP_OMP) ---------------------------- */
/* replaces pclomp::GeneralizedIterativeClosestPoint (include/ndt_omp/gicp_omp.h, gicp_omp_impl.hpp), the registration
 * select_registration_method hands out for registration_method = GICP_OMP (src/global_graph/registrations.cpp:43-53): one pair at a time,
 * synchronously, here; all candidates of a loop check in one lockstep batch below (mi355ndt_gicp_batch_*).  Three stages run on the device -- the k-nearest-neighbour covariances of both clouds (computeCovariances), the
 * correspondences with their Mahalanobis matrices, the cost / gradient sums -- and the BFGS optimiser and the outer loop of
 * computeTransformation run on the host, reading one small record per evaluation.  The rules are the reference's as restated in
 * tools/gicp_ref.py; FLANN's tie order, PCL's bfgs.h and Eigen's JacobiSVD are unpinned.
 * mi355ndt_gicp_params_default gives the constructor's values (gicp_omp.h:110-120): k_correspondences 20, gicp_epsilon 1e-3,
 * rotation_epsilon 2e-3, transformation_epsilon 5e-4, max_iterations 200, max_inner_iterations 20, corr_dist_threshold 5.0.  The factory
 * overrides four of them (registrations.cpp:47-51): transformation_epsilon 0.01, max_iterations 64, k_correspondences 20,
 * max_inner_iterations 20.  use_reciprocal_correspondences (false there) is not served.
 * Clouds: host records (x, y, z f32 first, stride_bytes apart) or resident keyframes by id.  A cloud's covariances are computed on first
 * use and kept until the cloud, k_correspondences or gicp_epsilon changes, as PCL keeps target_covariances_; a keyframe's stay with the
 * keyframe (72 B per point, beside the keyframe's one spatial index -- the one mi355ndt_keyframe_fitness_scores searches, built here if
 * that call has not built it; measured on a 65,536-point keyframe both surfaces have used: 128 B per point beside the rows) until
 * mi355ndt_keyframe_release, so the new keyframe of a loop check is decomposed once for all its candidates.  A released id is refused (MI355NDT_ERR_BAD_ARG) by the next call that needs the cloud.
 * Errors: MI355NDT_ERR_STATE in stream mode, and from the calls that need a cloud (or correspondences) that was not set (computed);
 * MI355NDT_ERR_BAD_ARG with a mi355ndt_last_error text for k_correspondences outside 1..64 or above the number of searchable points (three
 * finite coordinates) of a cloud -- the reference prints an error and reads unsized storage --, a NaN or negative epsilon or threshold,
 * negative iteration counts.  The batch, the grids, the keyframes' rows, the prefilter result and the other workspaces of the handle are left as they
 * were; fitness indexes are left as they were or built as the fitness surface would build them.
 *   role: MI355NDT_GICP_TARGET / MI355NDT_GICP_SOURCE.
 *   mi355ndt_gicp_covariances: n records of nine f64 (row-major 3x3), input order, zeros for a non-finite point; out may be NULL
 *     (compute and keep only); a count above capacity is MI355NDT_ERR_BAD_ARG.
 *   mi355ndt_gicp_correspondences: one pass of the matching loop (:415-466) with transformation_ = T (column-major f32; NULL: identity):
 *     idx (may be NULL) gets the target index per source point, -1 = none; maha (may be NULL) nine f64 per source point, zeros where
 *     unmatched; *m the number of matches.  The result stays resident for mi355ndt_gicp_cost.
 *   mi355ndt_gicp_cost: fdf (:343-378) over the resident correspondences at the state x[6] (x, y, z, roll, pitch, yaw) with base
 *     transformation `base`: *f and g[6] (either may be NULL).  MI355NDT_ERR_STATE with fewer than one match.
 *   mi355ndt_gicp_align: align(output, guess).  inner_status: the optimiser's last exit code (BFGSSpace::Status: -1 running, 0 success,
 *     1 no progress; -2 when it never ran); n_matched and delta: of the last outer iteration.
 *   mi355ndt_gicp_get_aligned: the source moved by the last final transformation, x, y, z into records of out_stride_bytes. */
enum { MI355NDT_GICP_TARGET = 0, MI355NDT_GICP_SOURCE = 1 };
typedef struct mi355ndt_gicp_params {
  int    k_correspondences;       /* setCorrespondenceRandomness      20   */
  double gicp_epsilon;            /* (no setter in the reference)     1e-3 */
  double rotation_epsilon;        /* setRotationEpsilon               2e-3 */
  double transformation_epsilon;  /* setTransformationEpsilon         5e-4 */
  int    max_iterations;          /* setMaximumIterations             200  */
  int    max_inner_iterations;    /* setMaximumOptimizerIterations    20   */
  double corr_dist_threshold;     /* setMaxCorrespondenceDistance     5.0  */
} mi355ndt_gicp_params;
typedef struct mi355ndt_gicp_result {
  float  final_colmajor[16];      /* getFinalTransformation(): [R_t R_g | t_t + t_g] (:508-511) */
  int    converged;               /* hasConverged() */
  int    iterations;              /* nr_iterations_: outer iterations */
  int    inner_status;
  int    n_matched;
  double delta;
} mi355ndt_gicp_result;
int mi355ndt_gicp_params_default(mi355ndt_gicp_params* p);
int mi355ndt_gicp_set_params(mi355ndt_handle* h, const mi355ndt_gicp_params* p);
int mi355ndt_gicp_set_target(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_gicp_set_source(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_gicp_set_target_keyframe(mi355ndt_handle* h, int id);
int mi355ndt_gicp_set_source_keyframe(mi355ndt_handle* h, int id);
int mi355ndt_gicp_covariances(mi355ndt_handle* h, int role, double* out, size_t capacity);
int mi355ndt_gicp_correspondences(mi355ndt_handle* h, const float* guess_colmajor, const float* T_colmajor, int* idx, double* maha, int* m);
int mi355ndt_gicp_cost(mi355ndt_handle* h, const double* x, const float* base_colmajor, double* f, double* g);
int mi355ndt_gicp_align(mi355ndt_handle* h, const float* guess_colmajor, mi355ndt_gicp_result* result);
int mi355ndt_gicp_get_aligned(mi355ndt_handle* h, void* out_pts, size_t out_stride_bytes);

/* ---- GICP, every candidate of a loop check in one lockstep batch ------------------------------------------------ */
/* The loop detector registers every candidate keyframe against the one new keyframe (loop_detector.hpp:148-205, :211-281).  The target is
 * the one mi355ndt_gicp_set_target / _set_target_keyframe set (setInputTarget(new_keyframe), once per loop check), the parameters are the
 * handle's mi355ndt_gicp_params; candidate k is the source of slot k.  mi355ndt_gicp_batch_align runs the K optimisers in lockstep: the
 * host keeps BFGS and the outer loop, one worker thread per slot, and every round ONE table copy, ONE matching launch, ONE cost launch,
 * ONE final launch and ONE wait serve all slots that wait for an evaluation -- the round trip is paid per round, not per candidate.
 * results[k] and mi355ndt_gicp_batch_get_aligned(k) are, byte for byte, what mi355ndt_gicp_set_source* + mi355ndt_gicp_align(guess k) +
 * mi355ndt_gicp_get_aligned give for that source against the same target.
 *   mi355ndt_gicp_batch_reserve: 1..MI355NDT_GICP_BATCH_MAX slots; drops the earlier slots.
 *   mi355ndt_gicp_batch_set_source / _set_source_keyframe: a host cloud (the slot owns its rows, index and covariances) or a resident
 *     keyframe (the keyframe's one index and its covariance cache are used, and filled; two slots may name the same keyframe).
 *   mi355ndt_gicp_batch_align: guesses n_slots x 16 floats (column-major 4x4 each), results n_slots records.
 *   mi355ndt_gicp_batch_stats: of the last batch align -- *rounds = the waits on the device, requests[k] (n_slots; may be NULL) = the
 *     device requests slot k made, a request being one matching pass or one cost evaluation.  rounds = the largest requests[k].
 * Errors: MI355NDT_ERR_STATE in stream mode, with no slots reserved, no target set or a slot unset; MI355NDT_ERR_BAD_ARG for a slot out of
 * range, n_slots outside 1..MI355NDT_GICP_BATCH_MAX, a released or unknown keyframe, and k_correspondences above a slot's searchable
 * points (the text names the slot).  A refused or failed call leaves the handle usable.  The single-pair surface (its two clouds, its resident
 * correspondences, its last final transformation), the NDT batch, the grids, the keyframes' rows and the other workspaces are left as they were. */
#define MI355NDT_GICP_BATCH_MAX 64
int mi355ndt_gicp_batch_reserve(mi355ndt_handle* h, int n_slots);
int mi355ndt_gicp_batch_set_source(mi355ndt_handle* h, int slot, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_gicp_batch_set_source_keyframe(mi355ndt_handle* h, int slot, int id);
int mi355ndt_gicp_batch_align(mi355ndt_handle* h, const float* guesses_colmajor, mi355ndt_gicp_result* results);
int mi355ndt_gicp_batch_get_aligned(mi355ndt_handle* h, int slot, void* out_pts, size_t out_stride_bytes);
int mi355ndt_gicp_batch_stats(mi355ndt_handle* h, int* rounds, int* requests);

/* ---- ICP: pcl::IterativeClosestPoint (registration_method = ICP) -------------------------------------------------- */
/* replaces pcl::IterativeClosestPoint as select_registration_method sets it up for registration_method = ICP
 * (src/global_graph/registrations.cpp:21-29: transformation_epsilon 0.01, maximum_iterations 64, use_reciprocal_correspondences false):
 * point-to-point ICP, one pair at a time, synchronously, here; all candidates of a loop check in one batch below (mi355ndt_icp_batch_*).
 * PCL is not part of the reference tree: computeTransformation, CorrespondenceEstimation, TransformationEstimationSVD (Eigen::umeyama
 * without scaling) and DefaultConvergenceCriteria are RESTATED AS RECALLED from PCL 1.8 (tools/icp_ref.py; parity unpinned,
 * INTEGRATION.md).  One iteration is one device round trip -- the working cloud is moved by the last estimate, matched against the target's
 * index and summed (two launches, one wait) -- and the host runs a 3x3 Jacobi SVD in f64 and the criteria on one small record.
 * What the engine fixes because PCL's is not reproducible or not observable: a tie in the nearest-point search goes to the lower point id;
 * d2 = (dx*dx + dy*dy) + dz*dz in f32; a correspondence is kept iff (double)d2 <= corr_dist_threshold^2; a source point that is not
 * finite, or whose moved copy is not finite, matches nothing; the centroid and covariance sums are f64 sums of f64 products of the f32
 * coordinates over a fixed tree (Eigen's are f32, in an order nobody can observe); the SVD is the engine's own (ndt_math.hpp jacobi_svd3).
 * PCL's slip is reproduced: the convergence test compares the SQUARED translation of an iteration with the unsquared
 * transformation_epsilon.  ICP reports hasConverged() = true at the iteration cap; so does this.
 * mi355ndt_icp_params_default gives pcl::Registration's constructor values: transformation_epsilon 0, max_iterations 10,
 * euclidean_fitness_epsilon -DBL_MAX, corr_dist_threshold sqrt(DBL_MAX), min_number_correspondences 3, use_reciprocal_correspondences 0.
 * use_reciprocal_correspondences != 0 is refused (it needs a search over the moving cloud every iteration: not served).
 * Clouds: host records or resident keyframes by id, as the GICP surface takes them; the target's one spatial index is the one the fitness
 * scores and GICP search (built here if they have not built it); a source needs none.  A keyframe source is never written: the working
 * cloud is the surface's own buffer.
 *   mi355ndt_icp_correspondences: one step on a fresh working cloud T (guess p) (two f32 products; T NULL: identity): idx (may be NULL)
 *     the target index per source point, -1 = none; d2 (may be NULL) the f32 squared distances, 0 where unmatched; sums (may be NULL)
 *     sixteen f64 over the matches, p the moved source point, q its target point: sum p [0..2], sum q [3..5], sum q_r p_c [6 + 3 r + c],
 *     sum d2 [15]; *m the matches.
 *   mi355ndt_icp_align: align(output, guess).  state: how the loop ended (mi355ndt_icp_state); matches and mse: of the last iteration.
 *   mi355ndt_icp_get_aligned: the working cloud after the last iteration's move (PCL's `output`), x, y, z into records of out_stride_bytes.
 * Errors: MI355NDT_ERR_STATE in stream mode and with a cloud unset; MI355NDT_ERR_BAD_ARG with a mi355ndt_last_error text for a NaN or
 * negative transformation_epsilon or corr_dist_threshold, a NaN euclidean_fitness_epsilon, a negative max_iterations or
 * min_number_correspondences, reciprocal correspondences, an empty cloud, a released keyframe.  The GICP and NDT surfaces, the batch, the
 * grids, the keyframes' rows and the other workspaces of the handle are left as they were. */
enum mi355ndt_icp_state {
  MI355NDT_ICP_NOT_CONVERGED = 0, MI355NDT_ICP_ITERATIONS = 1, MI355NDT_ICP_TRANSFORM = 2, MI355NDT_ICP_ABS_MSE = 3, MI355NDT_ICP_REL_MSE = 4,
  MI355NDT_ICP_NO_CORRESPONDENCES = 5
};
typedef struct mi355ndt_icp_params {
  double transformation_epsilon;         /* setTransformationEpsilon         0        */
  int    max_iterations;                 /* setMaximumIterations             10       */
  double euclidean_fitness_epsilon;      /* setEuclideanFitnessEpsilon       -DBL_MAX */
  double corr_dist_threshold;            /* setMaxCorrespondenceDistance     sqrt(DBL_MAX) */
  int    min_number_correspondences;     /* (no setter in PCL 1.8)           3        */
  int    use_reciprocal_correspondences; /* setUseReciprocalCorrespondences  0; != 0 is refused */
} mi355ndt_icp_params;
typedef struct mi355ndt_icp_result {
  float  final_colmajor[16];      /* getFinalTransformation() */
  int    converged;               /* hasConverged() */
  int    iterations;              /* nr_iterations_ */
  int    state;                   /* mi355ndt_icp_state */
  int    matches;                 /* correspondences of the last iteration */
  double mse;                     /* their mean squared distance (0 with none) */
} mi355ndt_icp_result;
int mi355ndt_icp_params_default(mi355ndt_icp_params* p);
int mi355ndt_icp_set_params(mi355ndt_handle* h, const mi355ndt_icp_params* p);
int mi355ndt_icp_set_target(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_icp_set_source(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_icp_set_target_keyframe(mi355ndt_handle* h, int id);
int mi355ndt_icp_set_source_keyframe(mi355ndt_handle* h, int id);
int mi355ndt_icp_correspondences(mi355ndt_handle* h, const float* guess_colmajor, const float* T_colmajor, int* idx, float* d2, double* sums, int* m);
int mi355ndt_icp_align(mi355ndt_handle* h, const float* guess_colmajor, mi355ndt_icp_result* result);
int mi355ndt_icp_get_aligned(mi355ndt_handle* h, void* out_pts, size_t out_stride_bytes);

/* ---- ICP, every candidate of a loop check in one batch ---------------------------------------------------------------- */
/* The target is the one mi355ndt_icp_set_target / _set_target_keyframe set, the parameters are the handle's mi355ndt_icp_params; candidate
 * k is the source of slot k.  ICP has no inner optimiser, so the batch is one loop on the calling thread (no worker threads): every round
 * ONE table copy, ONE step launch, ONE final launch and ONE wait serve all slots that have not ended, then each slot's SVD and criteria
 * run on the host; a slot that ended drops out of the table.  results[k] and mi355ndt_icp_batch_get_aligned(k) are, byte for byte, what
 * mi355ndt_icp_set_source* + mi355ndt_icp_align(guess k) + mi355ndt_icp_get_aligned give for that source against the same target.
 *   mi355ndt_icp_batch_reserve: 1..MI355NDT_ICP_BATCH_MAX slots; drops the earlier slots.
 *   mi355ndt_icp_batch_stats: of the last batch align -- *rounds = the waits on the device = the largest iteration count of a slot,
 *     requests[k] (n_slots; may be NULL) = the steps slot k took.
 * Errors: as the single-pair surface's; a slot out of range and n_slots out of range are MI355NDT_ERR_BAD_ARG; after a failed round nothing
 * more is launched and the first error is returned. */
#define MI355NDT_ICP_BATCH_MAX MI355NDT_GICP_BATCH_MAX
int mi355ndt_icp_batch_reserve(mi355ndt_handle* h, int n_slots);
int mi355ndt_icp_batch_set_source(mi355ndt_handle* h, int slot, const void* pts, size_t n, size_t stride_bytes);
int mi355ndt_icp_batch_set_source_keyframe(mi355ndt_handle* h, int slot, int id);
int mi355ndt_icp_batch_align(mi355ndt_handle* h, const float* guesses_colmajor, mi355ndt_icp_result* results);
int mi355ndt_icp_batch_get_aligned(mi355ndt_handle* h, int slot, void* out_pts, size_t out_stride_bytes);
int mi355ndt_icp_batch_stats(mi355ndt_handle* h, int* rounds, int* requests);

/* ---- exact k-nearest and radius search over resident keyframes ---------------------------------------------------- */
/* replaces pcl::KdTreeFLANN::nearestKSearch / radiusSearch over a keyframe a host would otherwise download (mi355ndt_keyframe_get) and
 * build a kd-tree over on the CPU: the search the fitness scores, ICP, the GICP covariances and the outlier removals run internally, as a
 * surface of its own, over the keyframe's one spatial index (found, whichever surface built it, or built here from
 * MI355NDT_OPT_KF_FITNESS_CELL_MM and kept until mi355ndt_keyframe_release; no result word depends on the cell size).  The rules are the
 * engine's, restated in tools/knn_ref.py:
 *   - searchable points: three finite coordinates; a keyframe without one (or without a point) gives count 0 everywhere;
 *   - the query: a point, moved by T_colmajor (4x4 f32; NULL: not moved) as ((T0 x + T1 y) + T2 z) + T3, every operation rounded on its
 *     own; a query that is not finite before or after the move finds nothing (count 0);
 *   - the distance: d2 = (dx*dx + dy*dy) + dz*dz in f32;
 *   - the order: ascending (d2, id): A TIE GOES TO THE LOWER POINT ID.  FLANN's order among equal distances is not observable and is
 *     not reproduced;
 *   - k-NN: the k first points in that order (1 <= k <= 64), kept iff (double)d2 <= max_range * max_range -- INCLUSIVE, ICP's rule;
 *     max_range +inf by default; counts[q] = the filled slots;
 *   - radius: within iff d2 < r2, r2 = (float)(radius * radius) -- STRICT, RadiusOutlierRemoval's rule and rounding; counts[q] = ALL the
 *     searchable points within, the lists hold the max_nn nearest of them (1 <= max_nn <= 64);
 *   - unused list slots: id -1, d2 +inf.
 * ids / d2 are [n][k] (or [n][max_nn]) row-major, counts [n].  query_order: how the queries are dealt to the lanes -- the input order, or
 * sorted by their cell in the searched keyframe's lattice (a wave's lanes then walk similar rings; one sort per item); both give identical
 * words.  MI355NDT_KNN_ORDER_AUTO follows the measurement in DESIGN.md section 8 (tools/keyframe_knn_timing.py): cell order for 4,096 or
 * more queries from the host (20-24 % faster when they arrive in no order, 0.05 ms slower when they are ordered already), input order
 * for fewer and for queries that are a resident keyframe (a window keyframe's points are in cell order as they are).
 * mi355ndt_keyframe_knn_ids: E (searched keyframe, query keyframe, pose) items in one launch chain and one wait, the queries read in
 * place (cloud_uploads does not move); relposes f64 [E][16] column-major, cast entry-wise to f32 as mi355ndt_keyframe_fitness_scores casts
 * them; the results are concatenated in item order; total_queries must equal the sum of the query keyframes' counts.
 * Errors, each with a message: MI355NDT_ERR_STATE in stream mode; MI355NDT_ERR_BAD_ARG for an unknown or released id, k or max_nn outside
 * 1..64, a NaN or negative max_range or radius, stride_bytes < 12, a NULL output, a wrong total_queries.  A refused call writes nothing,
 * changes nothing and builds nothing.  n == 0 and n_items == 0 are MI355NDT_OK with nothing written.  Synchronous, one wait for the
 * device per call; no keyframe is written. */
#define MI355NDT_KNN_ORDER_AUTO  0
#define MI355NDT_KNN_ORDER_INPUT 1
#define MI355NDT_KNN_ORDER_CELL  2
#define MI355NDT_KNN_MAX_K 64
typedef struct mi355ndt_knn_params {
  int    k;            /* 1 .. MI355NDT_KNN_MAX_K */
  double max_range;    /* >= 0; +inf: no limit */
  int    query_order;  /* MI355NDT_KNN_ORDER_* */
} mi355ndt_knn_params;
int mi355ndt_knn_params_default(mi355ndt_knn_params* p);   /* k 1, max_range +inf, query_order MI355NDT_KNN_ORDER_AUTO */
int mi355ndt_keyframe_knn(mi355ndt_handle* h, int kf_id, const void* queries, size_t n, size_t stride_bytes, const float* T_colmajor /* may be NULL */,
                          const mi355ndt_knn_params* p, int* ids /* [n][k] */, float* d2 /* [n][k] */, int* counts /* [n] */);
int mi355ndt_keyframe_knn_ids(mi355ndt_handle* h, int n_items, const int* searched_ids, const int* query_ids,
                              const double* relposes /* 16 per item, column-major f64 */, const mi355ndt_knn_params* p, size_t total_queries,
                              int* ids, float* d2, int* counts);
int mi355ndt_keyframe_radius_search(mi355ndt_handle* h, int kf_id, const void* queries, size_t n, size_t stride_bytes,
                                    const float* T_colmajor /* may be NULL */, double radius, int max_nn, int query_order,
                                    int* ids /* [n][max_nn] */, float* d2 /* [n][max_nn] */, int* counts /* [n] */);

/* profiling: HIP-event timing of the engine's own kernels on the engine's stream */
int mi355ndt_profile_enable(mi355ndt_handle* h, int on);
int mi355ndt_profile_reset(mi355ndt_handle* h);
int mi355ndt_profile_get(mi355ndt_handle* h, mi355ndt_profile* out);
int mi355ndt_synchronize(mi355ndt_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* MI355_NDT_H_ */
