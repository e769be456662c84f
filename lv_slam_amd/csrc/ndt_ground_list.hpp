// ndt_ground_list.hpp -- the gated sweep kernels of MI355NDT_OPT_GROUND_CLASS = 1 / 2 with the second f32 sum order (ORD = 1), compiled into
// mi355_ndt_ord1.hip beside the kernels of ndt_ord1_list.hpp; mi355_ndt.hip declares them `extern template`.  The list is the ORD = 1 row of
// ground_sweep_exists (ndt_sweep_exists.hpp) spelled out as text, because explicit instantiation needs that.  A change there is a change here.
#pragma once
#include "ndt_ord1_list.hpp"
// X(prefix) is expanded once per kernel: prefix = `extern template` or `template`
#define NDT_GROUND_ORD1_KERNELS(X)                                                                                                  \
  X __global__ void k_sweep<false, 1, 8, false, 1, 0, true> NDT_SWEEP_ARGS_T;  X __global__ void k_sweep<false, 7, 8, false, 1, 0, true> NDT_SWEEP_ARGS_T; \
  X __global__ void k_sweep<false, 26, 8, false, 1, 0, true> NDT_SWEEP_ARGS_T;
