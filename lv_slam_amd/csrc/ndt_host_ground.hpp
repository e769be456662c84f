// ndt_host_ground.hpp -- the launcher of the gated sweep kernels of MI355NDT_OPT_GROUND_CLASS = 1 / 2 (pclomp_ground, flag_class 1 / 2; ndt_sweep.hpp:
// GATE).  Included by ndt_host_sweep.hpp, whose launch_sweep calls it; the instantiations it names are the rows of ground_sweep_exists
// (ndt_sweep_exists.hpp), whose ORD = 1 half ndt_ground_list.hpp spells out for the second translation unit.
#pragma once

// the gated sweep of MI355NDT_OPT_GROUND_CLASS = 1 / 2: run-time (K, ord) -> its instantiation (ground_sweep_exists)
template <int K>
static void launch_sweep_ground_k(mi355ndt_handle* h, const SweepConst& sc, int ord, dim3 grid, SweepCtl* ctl, SweepCtl* ctl_next) {
  auto kern = ord == 1 ? k_sweep<false, K, SWEEP_IT_BATCH, false, 1, 0, true> : k_sweep<false, K, SWEEP_IT_BATCH, false, 0, 0, true>;
  kern<<<grid, SWEEP_THREADS, 0, h->stream>>>(h->d_src, h->src_pitch, h->d_state, h->d_grid, h->d_words, h->d_recs, h->d_partials, h->items_per_pair, h->d_active_list, ctl,
                                              ctl_next, sc, h->d_cent, h->d_grid_of_use);
}
static int launch_sweep_ground(mi355ndt_handle* h, const SweepConst& sc, int ord, dim3 grid, SweepCtl* ctl, SweepCtl* ctl_next) {
  if (sc.pca || h->fine_it || !ground_sweep_exists(sc.K, ord) || !sc.leaf_class || !h->built.made.leaf_class || (sc.gate_code != 1 && sc.gate_code != 2)) return MI355NDT_ERR_UNSUPPORTED;
  if (sc.K == 1) launch_sweep_ground_k<1>(h, sc, ord, grid, ctl, ctl_next);
  else if (sc.K == 7) launch_sweep_ground_k<7>(h, sc, ord, grid, ctl, ctl_next);
  else launch_sweep_ground_k<26>(h, sc, ord, grid, ctl, ctl_next);
  return MI355NDT_OK;
}
