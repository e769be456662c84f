// ndt_host_mapcloud.hpp -- mi355ndt_map_cloud: the global graph's map cloud (keyframe uploads, transform, octree codes, sort, emit).
#pragma once

// ---- map cloud ----------------------------------------------------------------------------------
// The map cloud has two routes to its keyframes and one way on from there: mi355ndt_map_cloud stages host clouds into d_mc_in,
// mi355ndt_map_cloud_keyframes (ndt_host_keyframe.hpp) reads the keyframe store.  Both size the workspace with mc_reserve, fill the McKf
// table in h_mc_tab (an address per keyframe) and hand over to mc_generate, which runs from the transform kernel to the output.
static int mc_reserve(mi355ndt_handle* h, int K, size_t n, size_t in_total) {
  hipStream_t s = h->stream;
  if (h->mc_pending) { HIPCHK(h, hipStreamSynchronize(s)); h->mc_pending = false; }
  const size_t pitch = (n + 63) & ~(size_t)63;
  const int nchunks = (int)((pitch + MC_CHUNK - 1) / MC_CHUNK);
  const int tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
  const int scan_chunks = (int)((pitch + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK);
  const size_t tab_bytes = (size_t)K * sizeof(McKf) + (size_t)K * 12 * sizeof(float);
  if (in_total > h->d_mc_in.cap || pitch > h->d_mc_pos.cap) {   // re-allocation: nothing of an earlier call may still run (uploads included)
    for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));
    HIPCHK(h, hipStreamSynchronize(s));
  }
  HIPCHK(h, h->d_mc_in.reserve(in_total)); HIPCHK(h, h->d_mc_x.reserve(3 * pitch)); HIPCHK(h, h->d_mc_out.reserve(3 * pitch));
  HIPCHK(h, h->d_mc_fin.reserve(pitch)); HIPCHK(h, h->d_mc_aabb.reserve(6 * (size_t)nchunks));
  HIPCHK(h, h->d_mc_keys.reserve(4 * pitch)); HIPCHK(h, h->d_mc_flag.reserve(pitch));
  HIPCHK(h, h->d_mc_hist.reserve((size_t)tiles << RS_MAX_BITS)); HIPCHK(h, h->d_mc_offs.reserve((size_t)tiles << RS_MAX_BITS));
  HIPCHK(h, h->d_mc_tmp.reserve((size_t)scan_chunks));
  HIPCHK(h, h->d_mc_kf.reserve((size_t)K)); HIPCHK(h, h->d_mc_T.reserve((size_t)K * 12)); HIPCHK(h, h->d_mc_box.reserve(1));
  HIPCHK(h, h->h_mc_tab.reserve(tab_bytes)); HIPCHK(h, h->h_mc_ret.reserve(4));
  HIPCHK(h, h->d_mc_pos.reserve(pitch));          // (last: its capacity vouches for the whole workspace above)
  return MI355NDT_OK;
}

static int mc_generate(mi355ndt_handle* h, int K, size_t n, const double* poses, double resolution, void* out_pts, size_t out_capacity,
                       size_t out_stride_bytes, size_t* n_out);

// replaces MapCloudGenerator::generate (src/global_graph/map_cloud_generator.cpp:17-55; global_graph_nodelet.cpp:725-745, 1036-1046): the
// keyframes' clouds go up through the engine's staging (up to UP_GROUP_MAX clouds per transfer, a few staging threads), one SoA row set per
// keyframe in a buffer of the map cloud's own; every kernel runs on the engine's stream and the call synchronises once, for the count.
int mi355ndt_map_cloud(mi355ndt_handle* h, int n_keyframes, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                       const double* poses, double resolution, void* out_pts, size_t out_capacity, size_t out_stride_bytes, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!n_out || n_keyframes < 0 || (out_pts && out_stride_bytes < 12)) return MI355NDT_ERR_BAD_ARG;
  *n_out = 0;
  if (n_keyframes == 0) return MI355NDT_OK;       // generate(): "keyframes empty" -> nullptr
  if (!(resolution > 0) || !std::isfinite(resolution) || !clouds || !counts || !poses) return MI355NDT_ERR_BAD_ARG;
  const int K = n_keyframes;
  size_t n = 0, in_total = 0;
  for (int k = 0; k < K; k++) {
    if ((counts[k] && !clouds[k]) || (counts[k] && stride_bytes < 12)) return MI355NDT_ERR_BAD_ARG;
    n += counts[k];
    in_total += 3 * ((counts[k] + 63) & ~(size_t)63);
    if (n >= (1u << 30)) return MI355NDT_ERR_BAD_ARG;   // (the prefilter's limit: int positions, 32-bit scan)
  }
  if (n == 0) return MI355NDT_OK;                 // no point at all: no octree leaf
  HIPCHK(h, hipSetDevice(h->device));
  int rc = mc_reserve(h, K, n, in_total);
  if (rc) return rc;

  McKf* kf = (McKf*)(unsigned char*)h->h_mc_tab;
  std::vector<UpItem> items;
  items.reserve((size_t)K);
  size_t start = 0, base = 0;
  for (int k = 0; k < K; k++) {
    const size_t kp = (counts[k] + 63) & ~(size_t)63;
    kf[k].rows = h->d_mc_in + base; kf[k].start = (unsigned)start; kf[k].pitch = (unsigned)kp;
    if (counts[k]) items.push_back(UpItem{h->d_mc_in + base, kp, 0, clouds[k], counts[k], stride_bytes});
    start += counts[k]; base += 3 * kp;
  }
  // the clouds: groups of up to UP_GROUP_MAX keyframes, one transfer each, staged by up to eight threads (the caller's among them)
  const int n_groups = (int)((items.size() + UP_GROUP_MAX - 1) / UP_GROUP_MAX);
  const int nt = std::max(1, std::min(8, n_groups));
  std::vector<int> rcs((size_t)nt, MI355NDT_OK);
  std::atomic<int> next_group{0};
  auto work = [&](int t) {
    (void)hipSetDevice(h->device);
    for (int g = next_group.fetch_add(1); g < n_groups; g = next_group.fetch_add(1)) {
      const size_t i0 = (size_t)g * UP_GROUP_MAX, i1 = std::min(items.size(), i0 + UP_GROUP_MAX);
      const int rc = upload_items(h, items.data() + i0, (int)(i1 - i0));
      if (rc != MI355NDT_OK) { rcs[(size_t)t] = rc; return; }
    }
  };
  std::vector<std::thread> th;
  try {
    th.reserve((size_t)nt);
    for (int t = 1; t < nt; t++) th.emplace_back(work, t);
  } catch (...) {}
  work(0);
  for (auto& x : th) x.join();
  for (int r : rcs) if (r != MI355NDT_OK) return r;
  return mc_generate(h, K, n, poses, resolution, out_pts, out_capacity, out_stride_bytes, n_out);
}

// From the transform kernel on.  h_mc_tab holds the McKf table of the K keyframes (n points in all); the poses become the f32 rows behind
// it (Matrix4f pose = keyframe->pose.matrix().cast<float>(), map_cloud_generator.cpp:31), one pinned block, two copies.
static int mc_generate(mi355ndt_handle* h, int K, size_t n, const double* poses, double resolution, void* out_pts, size_t out_capacity,
                       size_t out_stride_bytes, size_t* n_out) {
  hipStream_t s = h->stream;
  const size_t pitch = (n + 63) & ~(size_t)63;
  const int nchunks = (int)((pitch + MC_CHUNK - 1) / MC_CHUNK);
  const int tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
  const int scan_chunks = (int)((pitch + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK);
  McKf* kf = (McKf*)(unsigned char*)h->h_mc_tab;
  float* T = (float*)((unsigned char*)h->h_mc_tab + (size_t)K * sizeof(McKf));
  for (int k = 0; k < K; k++)
    for (int a = 0; a < 3; a++)
      for (int j = 0; j < 4; j++) T[12 * k + 4 * a + j] = (float)poses[16 * k + 4 * j + a];   // column-major f64 -> row-major f32 rows 0..2
  h->mc_pending = true;
  HIPCHK(h, hipMemcpyAsync(h->d_mc_kf, kf, (size_t)K * sizeof(McKf), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(h->d_mc_T, T, (size_t)K * 12 * sizeof(float), hipMemcpyHostToDevice, s));
  int rc = uploads_before_compute(h);
  if (rc) return rc;

  float* X = h->d_mc_x;
  unsigned *lo_a = h->d_mc_keys, *lo_b = lo_a + pitch, *hi_a = lo_b + pitch, *hi_b = hi_a + pitch;
  const int gx = (int)((pitch + 255) / 256);
  k_mc_transform<<<nchunks, MC_THREADS, 0, s>>>(h->d_mc_kf, K, h->d_mc_T, (int)n, pitch, X, h->d_mc_fin, h->d_mc_aabb);
  k_mc_box<<<1, MC_THREADS, 0, s>>>(X, pitch, h->d_mc_fin, h->d_mc_aabb, (int)n, resolution, h->d_mc_box);
  k_mc_keys<<<gx, 256, 0, s>>>(X, pitch, h->d_mc_fin, h->d_mc_box, resolution, lo_a, hi_a);
  // Stable LSD sort of the 64-bit codes with ndt_segsort.hpp's passes: the low words carrying the high words, then the high words carrying the
  // low words.  The final depth (3 * depth code bits) is only known on the device, so both words are sorted whole (3 + 3 passes of 11 bits):
  // reading it back first would cost a host round trip in the middle of the chain.
  const RsPlan plan = rs_plan(32);
  unsigned *kin = lo_a, *kout = lo_b, *vin = hi_a, *vout = hi_b;
  for (int p = 0; p < plan.passes; p++) {
    rs_pass(s, plan.bits, kin, vin, kout, vout, pitch, p * plan.bits, h->d_mc_hist, h->d_mc_offs, tiles, 1, false);
    std::swap(kin, kout); std::swap(vin, vout);
  }
  std::swap(kin, vin); std::swap(kout, vout);     // the high words become the keys
  for (int p = 0; p < plan.passes; p++) {
    rs_pass(s, plan.bits, kin, vin, kout, vout, pitch, p * plan.bits, h->d_mc_hist, h->d_mc_offs, tiles, 1, false);
    std::swap(kin, kout); std::swap(vin, vout);
  }
  const unsigned *hi_s = kin, *lo_s = vin;
  k_mc_heads<<<gx, 256, 0, s>>>(lo_s, hi_s, pitch, h->d_mc_flag);
  k_pf_scan_totals<<<scan_chunks, 1024, 0, s>>>(h->d_mc_flag, pitch, h->d_mc_tmp);
  k_pf_scan_offsets<<<1, 1024, 0, s>>>(h->d_mc_tmp, scan_chunks);
  k_pf_scan_apply<<<scan_chunks, 1024, 0, s>>>(h->d_mc_flag, pitch, h->d_mc_tmp, h->d_mc_pos);
  k_mc_emit<<<gx, 256, 0, s>>>(lo_s, hi_s, h->d_mc_flag, h->d_mc_pos, pitch, h->d_mc_box, resolution, h->d_mc_out);
  HIPCHK(h, hipGetLastError());
  int* ret = h->h_mc_ret;
  HIPCHK(h, hipMemcpyAsync(ret, &((McBox*)h->d_mc_box)->status, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(ret + 1, &((McBox*)h->d_mc_box)->depth, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(ret + 2, h->d_mc_pos + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(ret + 3, h->d_mc_flag + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  rc = compute_enqueued(h);                       // later uploads into the staging rows wait for these kernels
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  h->mc_pending = false;
  const int status = ret[0], depth = ret[1];
  if (status == MC_DEPTH) {
    h->err = "map_cloud: the points span more than 2^" + std::to_string(MC_MAX_DEPTH) + " voxels per axis at resolution " + std::to_string(resolution) +
             " (octree depth above " + std::to_string(MC_MAX_DEPTH) + ": the 63-bit Morton code of the engine cannot hold the keys)";
    return MI355NDT_ERR_BAD_ARG;
  }
  if (status == MC_ITERS) { h->err = "map_cloud: box growth did not finish within its round bound (depth " + std::to_string(depth) + ")"; return MI355NDT_ERR_HIP; }
  if (status == MC_EMPTY) return MI355NDT_OK;     // no finite point
  const size_t m = (size_t)ret[2] + (size_t)ret[3];
  *n_out = m;
  if (out_pts) {
    if (m > out_capacity) return MI355NDT_ERR_BAD_ARG;
    if (out_stride_bytes == 12) {
      if (m) HIPCHK(h, hipMemcpy(out_pts, h->d_mc_out, m * 12, hipMemcpyDeviceToHost));
    } else {
      std::vector<float> tmp(3 * m);
      if (m) HIPCHK(h, hipMemcpy(tmp.data(), h->d_mc_out, m * 12, hipMemcpyDeviceToHost));
      unsigned char* o = (unsigned char*)out_pts;
      for (size_t i = 0; i < m; i++) memcpy(o + i * out_stride_bytes, &tmp[3 * i], 12);
    }
  }
  return MI355NDT_OK;
}
