// ndt_grid_state.hpp -- the record of what the resident target grids hold (GridsBuilt), the one statement of what a configuration needs of
// them (grid_extras) and the one question asked of the record (grids_serve).  Nothing of HIP in this file: it compiles into the library's
// host side and into tests/cpp/grid_state_main.cpp.
#pragma once
#include "mi355_ndt.h"

// impl2:888: the More-Thuente loop (and computeHessian after it) runs iff !(step_max - step_min > 0), step_min = eps/2
static inline bool mt_is_live(const mi355ndt_params& p) { return !((p.step_size - p.trans_epsilon / 2) > 0); }
// ndt_pca + KDTREE: order-dependent weights -- its own per-leaf weights from the build (d_kdw), its own sweep kernel (ndt_sweep_kd.hpp)
static inline bool is_pca_kd(const mi355ndt_params& p) { return p.neighbor_mode == MI355NDT_KDTREE && p.variant == MI355NDT_VARIANT_PCA; }

// ---- MI355NDT_OPT_POSE_MODEL: 0 = ndt_omp_impl2.hpp (the SE(3) tangent), 1 = ndt_omp_impl.hpp (Euler angles).  What model 1 is served for is
// answered here and nowhere else: ndt_omp with the dead More-Thuente loop, the exact arithmetic (MI355NDT_OPT_ARITH is ignored), the plain lockstep
// rounds -- never the one-launch align, the latency pump, a sequence run or a stream.
enum { POSE_MODEL_SE3 = 0, POSE_MODEL_EULER = 1 };
// the arithmetic option as the engine's builds and sweeps see it
static inline int model_arith(int pose_model, int arith) { return pose_model == POSE_MODEL_EULER ? 0 : arith; }
// may an align of this model leave the lockstep rounds (one persistent launch, fine items)?
static inline bool model_leaves_rounds(int pose_model) { return pose_model != POSE_MODEL_EULER; }
// null: this model serves the configuration; else why not (MI355NDT_ERR_UNSUPPORTED)
static inline const char* model_refuses(const mi355ndt_params& p, int pose_model) {
  if (pose_model != POSE_MODEL_EULER) return nullptr;
  if (p.variant == MI355NDT_VARIANT_PCA) return "MI355NDT_OPT_POSE_MODEL = 1 serves variant = OMP alone (ndt_pca_impl.hpp has its weight commented out: it is ndt_omp's sweep)";
  if (mt_is_live(p)) return "MI355NDT_OPT_POSE_MODEL = 1 does not serve the live More-Thuente configuration (step_size <= trans_epsilon / 2)";
  return nullptr;
}

// what a target build can make beside the base records (grid descriptors, bitmap words, the exact voxel records)
struct GridExtras {
  bool cent;        // f32 leaf centroids: the KDTREE probe, computeHessian, calculateScore
  bool icov64;      // f64 inverse covariances: computeHessian, calculateScore
  bool kdw;         // per-leaf weights of ndt_pca + KDTREE (dead leaves included)
  bool recs_fast;   // the tolerance arithmetic's records (and, without centroids, its tree leaf sums)
  bool leaf_class = false;  // one class code per leaf record: the gated sweeps of MI355NDT_OPT_GROUND_CLASS = 1 / 2 (false wherever four entries are listed)
};
// What a configuration needs: a pure function of (parameters, MI355NDT_OPT_ARITH, live).  live: "as if the More-Thuente loop were live", the
// flavour calculateScore and computeHessian read whatever the configuration.  MI355NDT_OPT_ARITH = 1 is served for DIRECT1 / DIRECT7 with the dead
// More-Thuente loop (every configuration lv_slam ships); every other configuration ignores the option altogether: exact kernels, ordered leaf
// sums, the exact records alone.
static inline GridExtras grid_extras(const mi355ndt_params& p, int arith, bool live = false) {
  const bool mt_live = live || mt_is_live(p), direct_1_7 = p.neighbor_mode == MI355NDT_DIRECT1 || p.neighbor_mode == MI355NDT_DIRECT7;
  return {p.neighbor_mode == MI355NDT_KDTREE || mt_live, mt_live, is_pca_kd(p), arith == 1 && direct_1_7 && !mt_live};
}

struct GridsBuilt {
  bool valid;                   // the grids describe the target clouds the slots hold now
  GridExtras made;              // what the last build made beside the base records
  float leaf;                   // leaf size it used (setResolution without a source keeps the grids: ndt_omp.h:126-136)
  int cb;                       // cell-key bits it sorted
  size_t total_words;           // bitmap words of all its grids (a planned build of the stream: its plan's)
  bool fit_index;               // the fitness scores' occupied-cell index has been built over it (ndt_fitness.hpp)
};
// ---- MI355NDT_OPT_NDT_CLASS: 0 = pclomp::NormalDistributionsTransform (the option above says which implementation), 1 =
// pcl::NormalDistributionsTransform, PCL's own f64 class (registration_method = NDT, the factory's fall-back).  Class 1 is the Euler pose model
// with one neighbourhood -- radiusSearch(point, resolution), whatever neighbor_mode says -- and an f64 evaluation (ndt_sweep.hpp: eval_hit_pcl)
// that reads the leaves' f64 inverse covariances.  MI355NDT_OPT_POSE_MODEL and MI355NDT_OPT_ARITH are not consulted.  The overloads below take the
// class; the ones above are the class-0 answers.
enum { NDT_CLASS_OMP = 0, NDT_CLASS_PCL = 1 };
// the pose model an align of this class runs
static inline int class_model(int ndt_class, int pose_model) { return ndt_class == NDT_CLASS_PCL ? POSE_MODEL_EULER : pose_model; }
// the neighbour search an align of this class runs
static inline int class_neighbor_mode(int ndt_class, int neighbor_mode) { return ndt_class == NDT_CLASS_PCL ? (int)MI355NDT_KDTREE : neighbor_mode; }
static inline int model_arith(int pose_model, int arith, int ndt_class) { return model_arith(class_model(ndt_class, pose_model), arith); }
static inline bool model_leaves_rounds(int pose_model, int ndt_class) { return model_leaves_rounds(class_model(ndt_class, pose_model)); }
static inline const char* model_refuses(const mi355ndt_params& p, int pose_model, int ndt_class) {
  if (ndt_class != NDT_CLASS_PCL) return model_refuses(p, pose_model);
  if (p.variant == MI355NDT_VARIANT_PCA) return "MI355NDT_OPT_NDT_CLASS = 1 serves variant = OMP alone (pcl::NormalDistributionsTransform has no weights)";
  if (mt_is_live(p)) return "MI355NDT_OPT_NDT_CLASS = 1 does not serve the live More-Thuente configuration (step_size <= trans_epsilon / 2)";
  return nullptr;
}
// what a configuration of this class needs: class 1 reads the centroids (its radius search) and the f64 inverse covariances (its evaluation)
// whatever neighbor_mode says, and never the kd weights or the tolerance arithmetic's records
static inline GridExtras grid_extras(const mi355ndt_params& p, int arith, bool live, int ndt_class) {
  if (ndt_class != NDT_CLASS_PCL) return grid_extras(p, arith, live);
  return {true, true, false, false};
}

// ---- MI355NDT_OPT_GROUND_CLASS: 0 = none of it; 1 / 2 / 3 = pclomp_ground::NormalDistributionsTransformGround (ndt_ground_impl.hpp) with
// flag_class 1 (horizontal leaves; rows and columns 0, 1, 5 held), 2 (vertical leaves; 2, 3, 4 held), 0 (every point, nothing held).  The class is
// ndt_omp model 0 with a per-point gate on the class of the last neighbour, a doubled gradient and Hessian, the mask and a convergence test
// without the iteration guard.  What it is served for is answered by the overloads below and nowhere else: ndt_omp, the DIRECT searches, the dead
// More-Thuente loop, the exact arithmetic (MI355NDT_OPT_ARITH is ignored), the lockstep rounds.  Ground class 0 gives the answers above.
enum { GROUND_CLASS_NONE = 0, GROUND_CLASS_HORIZONTAL = 1, GROUND_CLASS_VERTICAL = 2, GROUND_CLASS_ALL = 3 };
static inline bool ground_class_valid(int ground) { return ground >= GROUND_CLASS_NONE && ground <= GROUND_CLASS_ALL; }
// does a sweep of this class gate its points (and read the leaves' class codes)?  Class 3 is the ungated ndt_omp sweep.
static inline bool ground_gated(int ground) { return ground == GROUND_CLASS_HORIZONTAL || ground == GROUND_CLASS_VERTICAL; }
static inline int model_arith(int pose_model, int arith, int ndt_class, int ground) { return ground != GROUND_CLASS_NONE ? 0 : model_arith(pose_model, arith, ndt_class); }
static inline bool model_leaves_rounds(int pose_model, int ndt_class, int ground) { return ground == GROUND_CLASS_NONE && model_leaves_rounds(pose_model, ndt_class); }
static inline const char* model_refuses(const mi355ndt_params& p, int pose_model, int ndt_class, int ground) {
  if (ground == GROUND_CLASS_NONE) return model_refuses(p, pose_model, ndt_class);
  if (ndt_class == NDT_CLASS_PCL) return "MI355NDT_OPT_GROUND_CLASS is not served together with MI355NDT_OPT_NDT_CLASS = 1 (pclomp_ground is built on pclomp's class)";
  if (pose_model == POSE_MODEL_EULER) return "MI355NDT_OPT_GROUND_CLASS is not served together with MI355NDT_OPT_POSE_MODEL = 1 (ndt_ground_impl.hpp is the SE(3) variant)";
  if (p.variant == MI355NDT_VARIANT_PCA) return "MI355NDT_OPT_GROUND_CLASS serves variant = OMP alone (pclomp_ground has no weights)";
  if (mt_is_live(p)) return "MI355NDT_OPT_GROUND_CLASS does not serve the live More-Thuente configuration (step_size <= trans_epsilon / 2): its computeHessian is unmasked";
  if (p.neighbor_mode == MI355NDT_KDTREE) return "MI355NDT_OPT_GROUND_CLASS serves DIRECT1 / DIRECT7 / DIRECT26 alone (the last neighbour of a radius search is FLANN's to order)";
  return nullptr;
}
// what a configuration of this class needs: the class-0 extras at the exact arithmetic, and the class codes where the sweep is gated
static inline GridExtras grid_extras(const mi355ndt_params& p, int arith, bool live, int ndt_class, int ground) {
  GridExtras e = grid_extras(p, ground != GROUND_CLASS_NONE ? 0 : arith, live, ndt_class);
  e.leaf_class = ground_gated(ground);
  return e;
}

static inline bool grids_serve(const GridsBuilt& b, const GridExtras& need) {
  return b.valid && (b.made.cent || !need.cent) && (b.made.icov64 || !need.icov64) && (b.made.kdw || !need.kdw) && (b.made.recs_fast || !need.recs_fast) &&
         (b.made.leaf_class || !need.leaf_class);
}
