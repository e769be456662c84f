// tools/lean_item_res.hip -- registers of the lean exact DIRECT7 item body (SweepTune<false, 7, ORD, true>, ndt_sweep.hpp) ALONE, full and score-only,
// at the lean kernel's launch bounds.  k_align_async's own figure includes the Newton update, whose local arrays live in scratch whatever the
// register budget; this wrapper holds nothing but the item, so "168 VGPRs, no scratch" can be read off the compiler's remarks.  Device code only,
// nothing to run:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fhip-fp32-correctly-rounded-divide-sqrt \
//         -mllvm -amdgpu-atomic-optimizer-strategy=None -Iinclude -Ilv_slam_amd/csrc -Rpass-analysis=kernel-resource-usage --cuda-device-only \
//         -c tools/lean_item_res.hip -o /dev/null 2> lean.log && python3 tools/kres.py lean.log 'k_lean_item|k_align_async'
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>
#include "mi355_ndt.h"
#include "ndt_math.hpp"
#include "ndt_types.hpp"
#include "ndt_sweep.hpp"
#include "ndt_newton.hpp"
#include "ndt_update.hpp"
#include "ndt_pose_record.hpp"
#include "ndt_async.hpp"
#include "ndt_sweep_exists.hpp"    // NDT_ASYNC_ARGS_T
// the lean item body alone, full and score-only, at the lean kernel's launch bounds
template <int ORD, bool SO>
__global__ void __launch_bounds__(SWEEP_THREADS, 3)
k_lean_item(int b, int rem, const float* __restrict__ src, size_t pitch, const PairState* st, const GridDesc* __restrict__ gd, const BitWord* __restrict__ words,
            const VoxelRec* __restrict__ recs, double* partials, int rows, SweepConst sc, const float* __restrict__ cent, int n) {
  __shared__ double exp_tab[64];
  if (threadIdx.x < 64) exp_tab[threadIdx.x] = ndtm::c_exp2_64[threadIdx.x];
  __syncthreads();
  Timeline tl;
  const unsigned pw = sweep_pose_words(st + b);
  sweep_item<false, 7, 8, false, ORD, true, SO, 0, true>(b, rem, src, pitch, st, gd, words, recs, partials, rows, sc, cent, nullptr, exp_tab, pw, n, b, tl);
}
template __global__ void k_lean_item<0, false>(int, int, const float*, size_t, const PairState*, const GridDesc*, const BitWord*, const VoxelRec*, double*, int, SweepConst, const float*, int);
template __global__ void k_lean_item<0, true>(int, int, const float*, size_t, const PairState*, const GridDesc*, const BitWord*, const VoxelRec*, double*, int, SweepConst, const float*, int);
template __global__ void k_lean_item<1, false>(int, int, const float*, size_t, const PairState*, const GridDesc*, const BitWord*, const VoxelRec*, double*, int, SweepConst, const float*, int);
template __global__ void k_lean_item<1, true>(int, int, const float*, size_t, const PairState*, const GridDesc*, const BitWord*, const VoxelRec*, double*, int, SweepConst, const float*, int);
// ... and the two kernels it is instantiated in, for comparison
template __global__ void k_align_async<false, 7, 0, true> NDT_ASYNC_ARGS_T;
template __global__ void k_align_async<false, 7, 0, false> NDT_ASYNC_ARGS_T;
