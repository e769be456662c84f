// tools/segsort_res.hip -- the segment sort's kernels (ndt_segsort.hpp) in a translation unit of their own, device code only, nothing to run: what
// each of them needs of a CU decides how many of its waves fit beside a running align launch.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fhip-fp32-correctly-rounded-divide-sqrt \
//         -mllvm -amdgpu-atomic-optimizer-strategy=None -Iinclude -Ilv_slam_amd/csrc -Rpass-analysis=kernel-resource-usage --cuda-device-only \
//         -c tools/segsort_res.hip -o /dev/null 2> segsort.log && python3 tools/slot_fit.py segsort.log
// tests/test_slot_fit_cpu.py holds k_rs_scatter to its budgets.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>
#include "ndt_segsort.hpp"
#define RS_INSTANTIATE(BITS)                                                                                                                       \
  template __global__ void k_rs_hist<BITS, false>(const unsigned*, size_t, int, unsigned*, int, int, const RsPoints);                              \
  template __global__ void k_rs_hist<BITS, true>(const unsigned*, size_t, int, unsigned*, int, int, const RsPoints);                               \
  template __global__ void k_rs_scan<BITS>(const unsigned*, unsigned*, int);                                                                       \
  template __global__ void k_rs_scatter<BITS, false>(const unsigned*, const unsigned*, unsigned*, unsigned*, size_t, int, const unsigned*, int, int); \
  template __global__ void k_rs_scatter<BITS, true>(const unsigned*, const unsigned*, unsigned*, unsigned*, size_t, int, const unsigned*, int, int);
RS_INSTANTIATE(8)
RS_INSTANTIATE(10)
RS_INSTANTIATE(11)
