// ndt_host_hooks.hpp -- parity hooks and getters: the aligned cloud, incremental transforms, derivatives / Hessian at a pose, grids and voxels,
// convertTransform, the NDT_TIMELINE read-outs.
#pragma once

int mi355ndt_get_aligned(mi355ndt_handle* h, void* out_pts, size_t stride) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!out_pts || stride < 12) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs < 1 || !h->d_src) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  { int rcu = uploads_before_compute(h); if (rcu) return rcu; }
  const int n = h->h_src_cnt[0];
  if (n == 0) return MI355NDT_OK;
  HIPCHK(h, h->d_aligned.reserve((size_t)3 * n));
  HIPCHK(h, h->h_pin_aligned.reserve((size_t)3 * n));
  // moved cloud as packed x,y,z triples -> pinned memory -> x,y,z of the caller's records (their other fields are left alone)
  k_transform<<<(n + 255) / 256, 256, 0, h->stream>>>(h->d_src, h->src_pitch, h->d_state, 0, h->d_aligned, n);
  HIPCHK(h, hipMemcpyAsync(h->h_pin_aligned, h->d_aligned, (size_t)3 * n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned char* o = (unsigned char*)out_pts;
  if (stride == 12) memcpy(o, h->h_pin_aligned, (size_t)n * 12);
  else for (int i = 0; i < n; i++) memcpy(o + (size_t)i * stride, h->h_pin_aligned + (size_t)3 * i, 12);
  return MI355NDT_OK;
}

int mi355ndt_get_incremental(mi355ndt_handle* h, int pair, float last[16], float prev[16]) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (pair < 0 || pair >= h->n_pairs) return MI355NDT_ERR_BAD_ARG;
  if (!h->d_state) return MI355NDT_ERR_STATE;
  if (!h->aligned_once) {                         // before any align(): transformation_ = previous_transformation_ = Identity
    for (int a = 0; a < 16; a++) { const float v = (a % 5 == 0) ? 1.f : 0.f; if (last) last[a] = v; if (prev) prev[a] = v; }
    return MI355NDT_OK;
  }
  HIPCHK(h, hipSetDevice(h->device));
  float buf[32];
  HIPCHK(h, hipMemcpyAsync(buf, (const char*)(h->d_state + pair) + offsetof(PairState, inc_cm), sizeof buf, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (last) memcpy(last, buf, 16 * sizeof(float));
  if (prev) memcpy(prev, buf + 16, 16 * sizeof(float));
  return MI355NDT_OK;
}

int mi355ndt_get_partial_rows(mi355ndt_handle* h, double* out, size_t capacity, int* rows_per_pair) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!rows_per_pair) return MI355NDT_ERR_BAD_ARG;
  if (h->n_pairs < 1 || !h->aligned_once || !h->d_partials || h->rows_per_pair < 1) return MI355NDT_ERR_STATE;
  *rows_per_pair = h->rows_per_pair;
  if (!out) return MI355NDT_OK;
  const size_t need = (size_t)h->n_pairs * h->rows_per_pair * NACC;
  if (capacity < need) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(out, h->d_partials, need * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MI355NDT_OK;
}

static int run_hook_sweep(mi355ndt_handle* h, double* score, double g[6], double H[36], long long* hits) {
  SweepConst sc;
  make_sweep_const(h, sc);
  int rc = launch_sweep(h, sc);
  if (rc) return rc;
  k_update<<<1, UPD_THREADS, 0, h->stream>>>(h->d_state, h->d_partials, h->rows_per_pair, h->pts_per_chunk, h->fine_it ? 1 : 0, h->d_results, h->d_active, h->d_active_list, h->d_ctl,
                                    nullptr, 0, 0, 0, 1, 0, nullptr, nullptr, eff_ground(h));
  PairState S;
  HIPCHK(h, hipMemcpyAsync(&S, h->d_state, sizeof(PairState), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  if (score) *score = S.score;
  if (g) memcpy(g, S.g, sizeof S.g);
  if (H) memcpy(H, S.H, sizeof S.H);
  if (hits) *hits = S.hits;
  return MI355NDT_OK;
}

static int hook_ready(mi355ndt_handle* h) {
  h->ev_last_fresh = false;
  if (h->n_pairs < 1 || !h->have_target || !h->have_source) return MI355NDT_ERR_STATE;
  const int rc = ensure_grids(h, GRIDS_CONFIG);
  return rc ? rc : prep_align_ws(h);
}

int mi355ndt_derivatives(mi355ndt_handle* h, const double p[6], double* score, double g[6], double H[36], long long* hits) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!p) return MI355NDT_ERR_BAD_ARG;
  // (model 1: p = [t; roll pitch yaw] -- the cloud is moved by convertTransform(p), the rows are taken from p: k_set_pose_p)
  if (const char* why = model_refuses(h->prm, h->pose_model, h->ndt_class, h->ground_class)) { h->err = why; return MI355NDT_ERR_UNSUPPORTED; }
  int rc = hook_ready(h);
  if (rc) return rc;
  double* dp = (double*)h->d_hook.p;
  HIPCHK(h, hipMemcpyAsync(dp, p, 6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_ctl, 0, 2 * sizeof(SweepCtl), h->stream));
  h->ctl_idx = 0;
  k_set_pose_p<<<1, 1, 0, h->stream>>>(h->d_state, 0, dp, h->d_src_cnt, h->d_grid, h->d_active_list, h->d_ctl, 0, euler_rows_of(h), pcl_rows_of(h));
  return run_hook_sweep(h, score, g, H, hits);
}

int mi355ndt_compute_hessian(mi355ndt_handle* h, const double p[6], double H[36]) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!p || !H) return MI355NDT_ERR_BAD_ARG;
  NOT_EULER(h, "mi355ndt_compute_hessian");             // (impl.hpp:913: dead at the settings model 1 serves)
  int rc = hook_ready(h);
  if (rc == MI355NDT_OK) rc = ensure_grids(h, GRIDS_LIVE);        // (the grid may have been built for a configuration that never needs the Hessian's inputs)
  if (rc) return rc;
  h->fine_it = 0; h->rows_per_pair = h->items_per_pair = h->chunks_per_pair * QUARTERS; h->pts_per_chunk = CHUNK_PTS;   // k_hessian writes batch-mode rows
  double* dp = (double*)h->d_hook.p;
  HIPCHK(h, hipMemcpyAsync(dp, p, 6 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_ctl, 0, 2 * sizeof(SweepCtl), h->stream));
  h->ctl_idx = 0;
  k_set_pose_p<<<1, 1, 0, h->stream>>>(h->d_state, 0, dp, h->d_src_cnt, h->d_grid, h->d_active_list, h->d_ctl, 1, nullptr, nullptr);
  SweepConst sc;
  make_sweep_const(h, sc);
  launch_hessian(h, sc);
  k_update<<<1, UPD_THREADS, 0, h->stream>>>(h->d_state, h->d_partials, h->rows_per_pair, h->pts_per_chunk, h->fine_it ? 1 : 0, h->d_results, h->d_active, h->d_active_list, h->d_ctl,
                                    nullptr, 0, 0, 0, 1, 2, nullptr, nullptr, 0);
  PairState S;
  HIPCHK(h, hipMemcpyAsync(&S, h->d_state, sizeof(PairState), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  memcpy(H, S.H, sizeof S.H);
  return MI355NDT_OK;
}

int mi355ndt_derivatives_T(mi355ndt_handle* h, const float T[16], const float Rj[9], double* score, double g[6], double H[36], long long* hits) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (!T || !Rj) return MI355NDT_ERR_BAD_ARG;
  NOT_EULER(h, "mi355ndt_derivatives_T");               // (the Euler model's sweep is a function of the pose vector: mi355ndt_derivatives)
  int rc = hook_ready(h);
  if (rc) return rc;
  float buf[25];
  memcpy(buf, T, 16 * sizeof(float));
  memcpy(buf + 16, Rj, 9 * sizeof(float));
  HIPCHK(h, hipMemcpyAsync(h->d_hook, buf, sizeof buf, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_ctl, 0, 2 * sizeof(SweepCtl), h->stream));
  h->ctl_idx = 0;
  k_set_pose<<<1, 1, 0, h->stream>>>(h->d_state, 0, h->d_hook, h->d_hook + 16, h->d_src_cnt, h->d_grid, h->d_active_list, h->d_ctl);
  return run_hook_sweep(h, score, g, H, hits);
}

// the descriptor of a pair's resident grid, for the two getters below
static int read_grid_desc(mi355ndt_handle* h, int pair, GridDesc& g) {
  if (!h->built.valid) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(&g, h->d_grid + pair, sizeof g, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return MI355NDT_OK;
}
int mi355ndt_get_grid(mi355ndt_handle* h, int pair, int min_b[3], int max_b[3], int div_b[3], int* n_voxels) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (pair < 0 || pair >= h->n_pairs) return MI355NDT_ERR_BAD_ARG;
  GridDesc g;
  if (int rc = read_grid_desc(h, pair, g)) return rc;
  for (int a = 0; a < 3; a++) {
    if (min_b) min_b[a] = g.min_b[a];
    if (max_b) max_b[a] = g.max_b[a];
    if (div_b) div_b[a] = g.div_b[a];
  }
  if (n_voxels) *n_voxels = g.n_voxels;
  return (g.status == GRID_OVERFLOW || g.status == GRID_CAP) ? MI355NDT_ERR_GRID : MI355NDT_OK;
}

int mi355ndt_get_voxels(mi355ndt_handle* h, int pair, mi355ndt_voxel* out, size_t capacity) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (pair < 0 || pair >= h->n_pairs || (!out && capacity)) return MI355NDT_ERR_BAD_ARG;
  GridDesc g;
  if (int rc = read_grid_desc(h, pair, g)) return rc;
  size_t n = std::min((size_t)g.n_voxels, capacity);
  if (n == 0) return MI355NDT_OK;
  std::vector<VoxelRec> r(n);
  std::vector<int> idx(n), cnt(n);
  HIPCHK(h, hipMemcpy(r.data(), h->d_recs + g.rec_off, n * sizeof(VoxelRec), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(idx.data(), h->d_vox_idx + g.rec_off, n * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(cnt.data(), h->d_vox_n + g.rec_off, n * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) {
    out[i].idx = idx[i];
    out[i].n = cnt[i];
    memcpy(out[i].mean, r[i].mean, sizeof r[i].mean);
    memcpy(out[i].icov, r[i].icov, sizeof r[i].icov);
    out[i].weight = (r[i].weight == VOX_DEAD) ? 0 : r[i].weight;
  }
  return MI355NDT_OK;
}

// One target's part of one buffer of the last synchronous build, raw, for the stage tests: nothing is launched, nothing on the device changes.
int mi355ndt_get_build_buffer(mi355ndt_handle* h, int which, int pair, void* out, size_t capacity_bytes, size_t* bytes) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!bytes || pair < 0 || pair >= h->n_pairs) return MI355NDT_ERR_BAD_ARG;
  *bytes = 0;
  GridDesc g;
  if (int rc = read_grid_desc(h, pair, g)) return rc;        // (ERR_STATE unless h->built.valid; waits for the stream)
  const size_t pitch = h->tgt_pitch, rpp = h->recs_per_pair, nv = (size_t)g.n_voxels;
  const unsigned nsl = ls_slices(pitch), scap = ls_slice_cap(h->prm.min_points_per_voxel);
  const GridExtras& made = h->built.made;
  const void* src = nullptr;
  size_t n = 0;
  unsigned long long geo[5];
  switch (which) {
    case MI355NDT_BUILD_MINMAX:    src = h->d_minmax + (size_t)pair * 6; n = 6 * sizeof(unsigned); break;
    case MI355NDT_BUILD_GRIDDESC:  src = &g; n = sizeof g; break;
    case MI355NDT_BUILD_WORDS:     src = h->d_words + g.word_off; n = (size_t)g.nwords * sizeof(BitWord); break;
    case MI355NDT_BUILD_KEYS:      src = h->d_keys_b + (size_t)pair * pitch; n = pitch * sizeof(unsigned); break;
    case MI355NDT_BUILD_IDS:       src = h->d_vals_b + (size_t)pair * pitch; n = pitch * sizeof(unsigned); break;
    case MI355NDT_BUILD_HEAD_CNT:  src = h->d_head_cnt + (size_t)pair * nsl; n = (size_t)nsl * sizeof(unsigned); break;
    case MI355NDT_BUILD_HEADS:     src = h->d_heads + (size_t)pair * nsl * scap; n = (size_t)nsl * scap * sizeof(unsigned); break;
    case MI355NDT_BUILD_SEG_START: src = h->d_seg_start + g.rec_off; n = nv * sizeof(unsigned); break;
    case MI355NDT_BUILD_SUMS:      src = h->d_sums + (size_t)g.rec_off * 9; n = nv * 9 * sizeof(double); break;
    case MI355NDT_BUILD_CENT:      if (!made.cent) return MI355NDT_ERR_BAD_ARG; src = h->d_cent + (size_t)g.rec_off * 3; n = nv * 3 * sizeof(float); break;
    case MI355NDT_BUILD_VOX_IDX:   src = h->d_vox_idx + g.rec_off; n = nv * sizeof(int); break;
    case MI355NDT_BUILD_VOX_N:     src = h->d_vox_n + g.rec_off; n = nv * sizeof(int); break;
    case MI355NDT_BUILD_ICOV64:    if (!made.icov64) return MI355NDT_ERR_BAD_ARG; src = h->d_icov64 + (size_t)g.rec_off * 9; n = nv * 9 * sizeof(double); break;
    case MI355NDT_BUILD_KD_WEIGHT: if (!made.kdw) return MI355NDT_ERR_BAD_ARG; src = h->d_kdw + g.rec_off; n = nv * sizeof(int); break;
    case MI355NDT_BUILD_LEAF_CLASS: if (!made.leaf_class) return MI355NDT_ERR_BAD_ARG; src = h->d_leaf_class + g.rec_off; n = nv * sizeof(unsigned char); break;
    case MI355NDT_BUILD_RECS_FAST: if (!made.recs_fast) return MI355NDT_ERR_BAD_ARG; src = h->d_recs_fast + g.rec_off; n = nv * sizeof(VoxelRecF); break;
    case MI355NDT_BUILD_SORTED_POINTS: if (!h->leaf_sorted || !h->d_sorted) return MI355NDT_ERR_BAD_ARG; src = h->d_sorted + (size_t)pair * pitch; n = pitch * sizeof(float4); break;
    case MI355NDT_BUILD_INFO:      src = h->d_word_off; n = 2 * sizeof(unsigned); break;
    case MI355NDT_BUILD_GEOMETRY:
      geo[0] = pitch; geo[1] = rpp; geo[2] = nsl; geo[3] = scap; geo[4] = (unsigned long long)h->built.cb;
      src = geo; n = sizeof geo; break;
    default: return MI355NDT_ERR_BAD_ARG;
  }
  *bytes = n;
  if (!out) return MI355NDT_OK;
  if (capacity_bytes < n) return MI355NDT_ERR_BAD_ARG;
  if (n == 0) return MI355NDT_OK;
  if (which == MI355NDT_BUILD_GRIDDESC || which == MI355NDT_BUILD_GEOMETRY) { memcpy(out, src, n); return MI355NDT_OK; }
  HIPCHK(h, hipMemcpy(out, src, n, hipMemcpyDeviceToHost));  // (the stream is idle: read_grid_desc waited for it)
  return MI355NDT_OK;
}

// replaces the static convertTransform helpers (ndt_omp.h:209-228); f32, the way Eigen 3.3 evaluates
// Translation3f * AngleAxisf(X) * AngleAxisf(Y) * AngleAxisf(Z) (third-party, restated from its published algorithm: AngleAxis::toRotationMatrix,
// Transform::rotate = linear() * R with coefficient-wise 3x3 products, a 3-term sum reduced as t0 + (t1 + t2))
static void aa_matrix(float angle, int axis, float R[9]) {
  const float ax[3] = {axis == 0 ? 1.f : 0.f, axis == 1 ? 1.f : 0.f, axis == 2 ? 1.f : 0.f};
  const float sn = sinf(angle), c = cosf(angle);
  const float sa[3] = {sn * ax[0], sn * ax[1], sn * ax[2]};
  const float c1[3] = {(1.f - c) * ax[0], (1.f - c) * ax[1], (1.f - c) * ax[2]};
  float tmp = c1[0] * ax[1];
  R[0 * 3 + 1] = tmp - sa[2]; R[1 * 3 + 0] = tmp + sa[2];
  tmp = c1[0] * ax[2];
  R[0 * 3 + 2] = tmp + sa[1]; R[2 * 3 + 0] = tmp - sa[1];
  tmp = c1[1] * ax[2];
  R[1 * 3 + 2] = tmp - sa[0]; R[2 * 3 + 1] = tmp + sa[0];
  for (int a = 0; a < 3; a++) R[a * 3 + a] = c1[a] * ax[a] + c;
}
static void mul33(const float A[9], const float B[9], float C[9]) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) C[r * 3 + c] = A[r * 3 + 0] * B[0 * 3 + c] + (A[r * 3 + 1] * B[1 * 3 + c] + A[r * 3 + 2] * B[2 * 3 + c]);
}
int mi355ndt_convert_transform(const double x[6], float out[16]) {
  if (!x || !out) return MI355NDT_ERR_BAD_ARG;
  float Rx[9], Ry[9], Rz[9], A[9], L[9];
  aa_matrix((float)x[3], 0, Rx); aa_matrix((float)x[4], 1, Ry); aa_matrix((float)x[5], 2, Rz);
  mul33(Rx, Ry, A);
  mul33(A, Rz, L);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) out[c * 4 + r] = L[r * 3 + c];
    out[12 + r] = (float)x[r];
    out[r * 4 + 3] = 0.f;
  }
  out[15] = 1.f;
  return MI355NDT_OK;
}

#ifdef NDT_TIMELINE
extern "C" int mi355ndt_debug_leaf_timeline(unsigned long long* out) {
  unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ltl), sizeof(z)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_ltl), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
extern "C" int mi355ndt_debug_timeline(unsigned long long* out) {
  unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl), sizeof(z)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_tl), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
#endif
