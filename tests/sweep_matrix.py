"""The kernel instantiations of the derivative sweep and of the one-launch align, as the lists the GPU tests iterate over
(tests/test_sweep_entries_gpu.py, tests/test_gpu_configs.py, tests/test_tiny_scene_models_gpu.py).  tests/test_sweep_entries_cpu.py holds these
lists to the one table of lv_slam_amd/csrc/ndt_sweep_exists.hpp: to its three row lists, to the predicates derived from them (sweep_exists,
euler_sweep_exists, ground_sweep_exists, lean_exists, align_exists) and to the kernels the built library holds.

pca: 0 = ndt_omp, 1 = ndt_pca.  K: cells probed -- 1 = DIRECT1, 7 = DIRECT7, 26 = DIRECT26, 27 = KDTREE.  ord: 0 / 1 = the exact arithmetic's two
f32 sum orders (MI355NDT_OPT_F32_SUM_ORDER), 2 = the tolerance arithmetic (MI355NDT_OPT_ARITH = 1).  it: 64-point tiles per work item, 8 = the
batch mode, 1 / 2 = the latency mode's fine items (MI355NDT_FINE_TILES)."""
IT_BATCH = 8
NAMES = {1: "direct1", 7: "direct7", 26: "direct26", 27: "kdtree"}

# k_sweep, SE(3) model: (pca, K, ord, it)
EXACT_BATCH = [(pca, K, ord, IT_BATCH) for pca in (0, 1) for K in (1, 7, 26) for ord in (0, 1)] + [(0, 27, ord, IT_BATCH) for ord in (0, 1)]
TOLERANCE_BATCH = [(pca, K, 2, IT_BATCH) for pca in (0, 1) for K in (1, 7)]
FINE = [(pca, K, ord, it) for pca in (0, 1) for K in (1, 7) for ord in (0, 1, 2) for it in (1, 2)]
SWEEP_ROWS = EXACT_BATCH + TOLERANCE_BATCH + FINE
# k_sweep_pca_kd<ord>: ndt_pca + KDTREE, the literal kernel
PCA_KD_ROWS = [0, 1]
# Euler-model k_sweep: (K, ord)
EULER_ROWS = [(K, ord) for K in (1, 7, 26, 27) for ord in (0, 1)]
# PCL's f64 class: k_sweep<false, 27, 8, false, 0, 2> -- (K, ord)
PCL_ROWS = [(27, 0)]
# the gated k_sweep of MI355NDT_OPT_GROUND_CLASS = 1 / 2: (K, ord)
GROUND_ROWS = [(K, ord) for K in (1, 7, 26) for ord in (0, 1)]
# k_align_async: (pca, K, ord, lean)
ALIGN_ROWS = [(pca, K, ord, 0) for pca, K, ord, _ in EXACT_BATCH + TOLERANCE_BATCH] + [(0, 7, 0, 1), (0, 7, 1, 1)]

assert (len(EXACT_BATCH), len(TOLERANCE_BATCH), len(FINE), len(SWEEP_ROWS)) == (14, 4, 24, 42)
assert len(SWEEP_ROWS) + len(EULER_ROWS) + len(PCL_ROWS) + len(GROUND_ROWS) == 57
assert len(SWEEP_ROWS) + len(EULER_ROWS) + len(PCL_ROWS) + len(GROUND_ROWS) + len(PCA_KD_ROWS) + len(ALIGN_ROWS) == 79


def row_id(row):
    pca, K, ord_, last = row
    return f"{'pca' if pca else 'omp'}_{NAMES[K]}_{('ord0', 'ord1', 'tol')[ord_]}_{last}"
