// ndt_host_life.hpp -- create / destroy, device and NUMA queries, parameters (mi355ndt_set_params: when the grids are re-made), options,
// stream binding, synchronize.
#pragma once

const char* mi355ndt_version(void) { return "mi355ndt 0.1 (gfx950)"; }

int mi355ndt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// NUMA node of the host CPUs closest to `device` (-1: unknown) -- staging threads and the clouds they read belong there
int mi355ndt_host_numa_node(int device) {
  int node = -1;
  if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, device) != hipSuccess) {
    (void)hipGetLastError();                      // not every runtime answers this attribute: leave no sticky error behind
    // fall back to the PCI device's sysfs entry
    char bdf[64];
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char* c = bdf; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    std::ifstream f(std::string("/sys/bus/pci/devices/") + bdf + "/numa_node");
    if (f && (f >> node)) return node;
    // containers usually hide the PCI tree but show the KFD topology: find the GPU node by its PCI location, then the CPU node
    // that has an io_link to it (KFD numbers its CPU nodes like the NUMA nodes)
    unsigned dom = 0, bus = 0, dv = 0, fn = 0;
    if (sscanf(bdf, "%x:%x:%x.%x", &dom, &bus, &dv, &fn) != 4) return -1;
    const long want = (long)((bus << 8) | (dv << 3) | fn);
    auto prop = [](const std::string& path, const char* key, long& out) {
      std::ifstream pf(path);
      std::string k; long v;
      while (pf >> k >> v) if (k == key) { out = v; return true; }
      return false;
    };
    const std::string top = "/sys/class/kfd/kfd/topology/nodes/";
    int gpu_node = -1;
    for (int n = 0; n < 64 && gpu_node < 0; n++) {
      long loc = -1, simd = 0;
      if (prop(top + std::to_string(n) + "/properties", "simd_count", simd) && simd > 0 &&
          prop(top + std::to_string(n) + "/properties", "location_id", loc) && loc == want) gpu_node = n;
    }
    if (gpu_node < 0) return -1;
    node = -1;
    for (int n = 0; n < 64 && node < 0; n++) {
      long cores = 0;
      if (!prop(top + std::to_string(n) + "/properties", "cpu_cores_count", cores) || cores <= 0) continue;
      for (int l = 0; l < 64; l++) {
        long to = -1;
        if (!prop(top + std::to_string(n) + "/io_links/" + std::to_string(l) + "/properties", "node_to", to)) break;
        if (to == gpu_node) { node = n; break; }
      }
    }
  }
  return node;
}

// CPUs of a NUMA node as an affinity mask (empty on failure)
static bool numa_cpus(int node, cpu_set_t* set) {
  CPU_ZERO(set);
  if (node < 0) return false;
  std::ifstream f("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
  std::string txt;
  if (!f || !std::getline(f, txt)) return false;
  bool any = false;
  size_t pos = 0;
  while (pos < txt.size()) {
    size_t comma = txt.find(',', pos);
    std::string part = txt.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
    size_t dash = part.find('-');
    int lo = atoi(part.c_str()), hi = dash == std::string::npos ? lo : atoi(part.c_str() + dash + 1);
    for (int c = lo; c <= hi && c < CPU_SETSIZE; c++) { CPU_SET(c, set); any = true; }
    if (comma == std::string::npos) break;
    pos = comma + 1;
  }
  return any;
}

int mi355ndt_default_params(mi355ndt_params* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  p->resolution = 1.0f;
  p->step_size = 0.1;
  p->outlier_ratio = 0.55;
  p->trans_epsilon = 0.1;
  p->max_iterations = 35;
  p->neighbor_mode = MI355NDT_DIRECT7;
  p->variant = MI355NDT_VARIANT_OMP;
  p->min_points_per_voxel = 6;
  p->min_covar_eigvalue_mult = 0.01;
  return MI355NDT_OK;
}

int mi355ndt_create(const mi355ndt_params* params, int device, mi355ndt_handle** out) {
  if (!out) return MI355NDT_ERR_BAD_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MI355NDT_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return MI355NDT_ERR_BAD_ARG;
  mi355ndt_params p;
  mi355ndt_default_params(&p);
  if (params) p = *params;
  int rc = check_params(p);
  if (rc) return rc;
  std::unique_ptr<mi355ndt_handle> h(new mi355ndt_handle());   // (a failure below releases whatever was created before it)
  h->device = device;
  h->prm = p;
  gauss_constants3(0.55, 1.0f, h->gauss_last);    // the constructor's gauss_d*_ (impl2:70-76: resolution_ 1.0f, outlier_ratio_ 0.55), whatever the setters say later
  { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) h->n_cu = pr.multiProcessorCount; }
  if (const char* e = std::getenv("MI355NDT_LEAF_SORTED")) h->leaf_sorted = std::atoi(e) != 0;
  if (const char* e = std::getenv("MI355NDT_FINE_TILES")) { const int v = std::atoi(e); if (v == 1 || v == 2) h->fine_tiles = v; }
  if (const char* e = std::getenv("MI355NDT_ARITH")) h->arith = std::atoi(e) == 1 ? 1 : 0;   // default of MI355NDT_OPT_ARITH for engines created afterwards (tools, A/B runs)
  if (const char* e = std::getenv("MI355NDT_SWEEP_WAVES")) { const int v = std::atoi(e); if (v == 0 || v == 2 || v == 3) h->sweep_waves = v; }   // default of MI355NDT_OPT_SWEEP_WAVES (A/B runs)
  if (const char* e = std::getenv("MI355NDT_ASYNC")) { h->async_align = std::atoi(e) != 0; h->async_force = std::atoi(e) == 2; }
  if (const char* e = std::getenv("MI355NDT_SCORE_ONLY_LAST_SWEEP")) h->score_only_last = std::atoi(e) != 0;   // default of MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP (A/B runs)
  if (const char* e = std::getenv("MI355NDT_SWEEP_DYN_SHIFT")) { const int v = std::atoi(e); if (v >= 0 && v <= 30) h->dyn_shift = v; }
  if (hipSetDevice(device) != hipSuccess || h->own_stream.create() != hipSuccess) return MI355NDT_ERR_HIP;
  h->stream = h->own_stream;
  if (h->h_pin_u.realloc_exact(4) != hipSuccess ||
      h->h_pin_active.realloc_exact(128) != hipSuccess ||
      h->d_active.realloc_exact(128) != hipSuccess ||
      h->d_ctl.realloc_exact(2) != hipSuccess ||
      h->d_hits.realloc_exact(2) != hipSuccess ||
      hipMemsetAsync(h->d_hits, 0, 2 * sizeof(unsigned long long), h->stream) != hipSuccess ||   // (the counters start at zero, not at what the allocation held)
      h->d_hook.realloc_exact(64 * sizeof(double) / sizeof(float)) != hipSuccess ||
      h->ev_compute.create() != hipSuccess || h->ev_burst[0].create() != hipSuccess || h->ev_burst[1].create() != hipSuccess) return MI355NDT_ERR_HIP;
  for (int i = 0; i < mi355ndt_handle::UP_STREAMS; i++)
    if (h->copy_stream[i].create() != hipSuccess || h->ev_uploads[i].create() != hipSuccess) return MI355NDT_ERR_HIP;
  *out = h.release();
  return MI355NDT_OK;
}

int mi355ndt_destroy(mi355ndt_handle* h) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (h->ss) (void)mi355ndt_stream_end(h);
  for (hipStream_t cs : h->copy_stream) if (cs) (void)hipStreamSynchronize(cs);
  delete h;                                       // (the owners release every buffer, block, event and stream)
  return MI355NDT_OK;
}

int mi355ndt_get_params(const mi355ndt_handle* h, mi355ndt_params* out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!out) return MI355NDT_ERR_BAD_ARG;
  *out = h->prm;
  return MI355NDT_OK;
}

int mi355ndt_set_stream(mi355ndt_handle* h, void* s) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  if (s) {
    h->own_stream.reset();
    h->stream = (hipStream_t)s;
  } else if (!h->own_stream) {
    HIPCHK(h, h->own_stream.create());
    h->stream = h->own_stream;
  }
  return MI355NDT_OK;
}

const char* mi355ndt_last_error(const mi355ndt_handle* h) { return h ? h->err.c_str() : "bad handle"; }

int mi355ndt_synchronize(mi355ndt_handle* h) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  HIPCHK(h, hipSetDevice(h->device));
  // uploads are asynchronous on the copy streams: "everything issued so far is done" includes them (and a failed transfer
  // surfaces here, not in an unrelated later call)
  for (hipStream_t cs : h->copy_stream) if (cs) HIPCHK(h, hipStreamSynchronize(cs));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MI355NDT_OK;
}

int mi355ndt_batch_size(const mi355ndt_handle* h) { return h ? h->n_pairs : MI355NDT_ERR_BAD_HANDLE; }

int mi355ndt_set_params(mi355ndt_handle* h, const mi355ndt_params* p) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!p) return MI355NDT_ERR_BAD_ARG;
  int rc = check_params(*p);
  if (rc) return rc;
  const mi355ndt_params old = h->prm;
  h->prm = *p;
  // setResolution (ndt_omp.h:126-136): `if (resolution_ != resolution) { resolution_ = resolution; if (input_) init(); }` -- the grid is only
  // re-made when a SOURCE cloud is set; without one it keeps its leaf size until the next setInputTarget, while the Gauss constants follow
  // the new value (impl2:93-100).  Reproduced for the DIRECT searches of the single-registration surface; a radius search over the grid
  // (KDTREE, live More-Thuente) is emulated by a 27-cell probe that needs radius <= leaf, so those re-voxelise as before (documented deviation).
  const bool radius_search = class_neighbor_mode(h->ndt_class, p->neighbor_mode) == MI355NDT_KDTREE || mt_is_live(*p);
  const bool keep_grid = old.resolution != p->resolution && h->n_pairs == 1 && !h->have_source && !radius_search && h->d_tgt == h->d_tgt_own;
  const bool regrid = (old.resolution != p->resolution && !keep_grid) || old.variant != p->variant ||
                      old.min_points_per_voxel != p->min_points_per_voxel ||
                      old.min_covar_eigvalue_mult != p->min_covar_eigvalue_mult ||
                      !grids_serve(h->built, grid_extras(*p, 0, false, h->ndt_class));   // centroids, f64 inverse covariances or kd weights the build skipped (arith 0: the
                                                                    // tolerance arithmetic's records are left to the next align)
  if (regrid && h->built.valid) {
    h->built.valid = false;
    rc = ensure_grids(h, GRIDS_CONFIG);       // setResolution -> init() (ndt_omp.h:126-136)
    if (rc) h->prm = old;                     // the grids were not rebuilt: keep the parameters they were (last) built with;
    return rc;                                // built.valid stays false, so the next align re-voxelises
  }
  return MI355NDT_OK;
}

int mi355ndt_set_option(mi355ndt_handle* h, int option, int value) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  // (what a stream's launches and its contexts' synchronous re-runs compute with was fixed at mi355ndt_stream_begin: not changed mid-stream)
  if (h->ss && (option == MI355NDT_OPT_F32_SUM_ORDER || option == MI355NDT_OPT_ARITH || option == MI355NDT_OPT_ASYNC_ALIGN ||
                       option == MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP || option == MI355NDT_OPT_POSE_MODEL || option == MI355NDT_OPT_NDT_CLASS || option == MI355NDT_OPT_GROUND_CLASS ||
                       option == MI355NDT_OPT_SWEEP_WAVES)) NOT_IN_STREAM(h);
  if (option == MI355NDT_OPT_GROUND_CLASS) {
    if (!ground_class_valid(value)) return MI355NDT_ERR_BAD_ARG;
    h->ground_class = value;                     // (what it serves and needs of the grids: ndt_grid_state.hpp; the next align builds the class codes a resident target lacks)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_NDT_CLASS) {
    if (value != NDT_CLASS_OMP && value != NDT_CLASS_PCL) return MI355NDT_ERR_BAD_ARG;
    h->ndt_class = value;                        // (what class 1 serves and needs of the grids: ndt_grid_state.hpp; the next align rebuilds what a resident target lacks)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_POSE_MODEL) {
    if (value != POSE_MODEL_SE3 && value != POSE_MODEL_EULER) return MI355NDT_ERR_BAD_ARG;
    h->pose_model = value;                       // (what model 1 serves: ndt_grid_state.hpp; grids built for the tolerance arithmetic are rebuilt by the next align)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_F32_SUM_ORDER) {
    if (value != 0 && value != 1) return MI355NDT_ERR_BAD_ARG;
    h->f32_sum_order = value;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_ARITH) {
    if (value != 0 && value != 1) return MI355NDT_ERR_BAD_ARG;
    h->arith = value;                            // (grids built before lack the records of the other arithmetic: the next align rebuilds them)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_SWEEP_WAVES) {
    if (const int rc = sweep_waves_option_rc(false, value)) return rc;     // (a stream: refused above)
    h->sweep_waves = value;                      // (no result word depends on it: which body serves a launch is decided per launch, async_lean)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_ASYNC_ALIGN) {
    if (value < 0 || value > 2) return MI355NDT_ERR_BAD_ARG;
    h->async_align = value != 0;
    h->async_force = value == 2;                 // 2: also for batches smaller than the GPU's resident waves (testing)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP) {
    if (value != 0 && value != 1) return MI355NDT_ERR_BAD_ARG;
    h->score_only_last = value;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_DEBUG_ASYNC_ABORT) {
    h->debug_abort_pos = value < 0 ? 0xFFFFFFFFu : (unsigned)value;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_DEBUG_ASYNC_RINGS) {
    if ((value & 0xFF) == 0) return MI355NDT_ERR_BAD_ARG;
    h->debug_ring_mask = (unsigned)value & 0xFFu;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_STREAM_THRESHOLD) {
    if (value < -1 || value > ASYNC_MAX_CARRY) return MI355NDT_ERR_BAD_ARG;
    h->s_thresh_opt = value;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_STREAM_RESERVE) {
    if (value < -1 || value > 4096) return MI355NDT_ERR_BAD_ARG;
    h->s_reserve_opt = value;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_KF_FITNESS_CELL_MM) {
    if (value < 1 || value > 1000000) return MI355NDT_ERR_BAD_ARG;
    h->kff_cell_mm = value;                      // (indexes that exist keep the cell they were built with)
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_OUTLIER_CELL_MM) {
    if (value < 1 || value > 1000000) return MI355NDT_ERR_BAD_ARG;
    h->ol_cell_mm = value;
    return MI355NDT_OK;
  }
  if (option == MI355NDT_OPT_PREFILTER_GROUP) {
    if (value < 0 || value > 4096) return MI355NDT_ERR_BAD_ARG;
    h->pf_group = value;
    return MI355NDT_OK;
  }
  return MI355NDT_ERR_BAD_ARG;
}
int mi355ndt_get_option(const mi355ndt_handle* h, int option, int* value) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!value) return MI355NDT_ERR_BAD_ARG;
  if (option == MI355NDT_OPT_F32_SUM_ORDER) { *value = h->f32_sum_order; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_ARITH) { *value = h->arith; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_SWEEP_WAVES) { *value = h->sweep_waves; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_POSE_MODEL) { *value = h->pose_model; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_NDT_CLASS) { *value = h->ndt_class; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_GROUND_CLASS) { *value = h->ground_class; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_ASYNC_ALIGN) { *value = h->async_force ? 2 : (h->async_align ? 1 : 0); return MI355NDT_OK; }
  if (option == MI355NDT_OPT_SCORE_ONLY_LAST_SWEEP) { *value = h->score_only_last; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_DEBUG_ASYNC_ABORT) { *value = h->debug_abort_pos == 0xFFFFFFFFu ? -1 : (int)h->debug_abort_pos; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_DEBUG_ASYNC_RINGS) { *value = (int)h->debug_ring_mask; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_STREAM_THRESHOLD) { *value = h->s_thresh_opt; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_STREAM_RESERVE) { *value = h->s_reserve_opt; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_KF_FITNESS_CELL_MM) { *value = h->kff_cell_mm; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_OUTLIER_CELL_MM) { *value = h->ol_cell_mm; return MI355NDT_OK; }
  if (option == MI355NDT_OPT_PREFILTER_GROUP) { *value = h->pf_group; return MI355NDT_OK; }
  return MI355NDT_ERR_BAD_ARG;
}
