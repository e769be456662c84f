// ndt_host_mapcloud.hpp -- mi355ndt_map_cloud: the global graph's map cloud (keyframe uploads, transform, octree codes, sort, emit).
#pragma once

// ---- map cloud ----------------------------------------------------------------------------------
// The map cloud has two routes to its keyframes and one way on from there: mi355ndt_map_cloud stages host clouds into the scratch's `in`,
// mi355ndt_map_cloud_keyframes (ndt_host_keyframe.hpp) reads the keyframe store.  Both size the scratch with mc_reserve, fill the McKf
// table in its pinned block (an address per keyframe) and hand over to mc_generate, which runs from the transform kernel to the output.
static int mc_reserve(mi355ndt_handle* h, int K, size_t n, size_t in_total) {
  VsNeed need;
  need.pitch = (n + 63) & ~(size_t)63; need.in = in_total; need.x = need.out = 3 * need.pitch;
  need.tab = (size_t)K * sizeof(McKf) + (size_t)K * 12 * sizeof(float);
  return vs_reserve(h, need);
}

static int mc_generate(mi355ndt_handle* h, int K, size_t n, const double* poses, double resolution, void* out_pts, size_t out_capacity,
                       size_t out_stride_bytes, size_t* n_out);

// replaces MapCloudGenerator::generate (src/global_graph/map_cloud_generator.cpp:17-55; global_graph_nodelet.cpp:725-745, 1036-1046): the
// keyframes' clouds go up through the engine's staging (up to UP_GROUP_MAX clouds per transfer, a few staging threads), one SoA row set per
// keyframe in the shared scratch; every kernel runs on the engine's stream and the call synchronises once, for the count.
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

  VoxelScratch& w = h->vs;
  McKf* kf = (McKf*)(unsigned char*)w.h_tab;
  std::vector<UpItem> items;
  items.reserve((size_t)K);
  size_t start = 0, base = 0;
  for (int k = 0; k < K; k++) {
    const size_t kp = (counts[k] + 63) & ~(size_t)63;
    kf[k].rows = w.in + base; kf[k].start = (unsigned)start; kf[k].pitch = (unsigned)kp;
    if (counts[k]) items.push_back(UpItem{w.in + base, kp, 0, clouds[k], counts[k], stride_bytes});
    start += counts[k]; base += 3 * kp;
  }
  rc = upload_items_grouped(h, items);
  if (rc) return rc;
  return mc_generate(h, K, n, poses, resolution, out_pts, out_capacity, out_stride_bytes, n_out);
}

// From the transform kernel on.  The scratch's pinned block holds the McKf table of the K keyframes (n points in all); the poses become the
// f32 rows behind it (Matrix4f pose = keyframe->pose.matrix().cast<float>(), map_cloud_generator.cpp:31), and the block goes over as one copy.
static int mc_generate(mi355ndt_handle* h, int K, size_t n, const double* poses, double resolution, void* out_pts, size_t out_capacity,
                       size_t out_stride_bytes, size_t* n_out) {
  VoxelScratch& w = h->vs;
  hipStream_t s = h->stream;
  const size_t pitch = (n + 63) & ~(size_t)63;
  const int nchunks = (int)((pitch + MC_CHUNK - 1) / MC_CHUNK);
  const size_t at_T = (size_t)K * sizeof(McKf);
  float* T = (float*)((unsigned char*)w.h_tab + at_T);
  for (int k = 0; k < K; k++)
    for (int a = 0; a < 3; a++)
      for (int j = 0; j < 4; j++) T[12 * k + 4 * a + j] = (float)poses[16 * k + 4 * j + a];   // column-major f64 -> row-major f32 rows 0..2
  w.pending = true;
  HIPCHK(h, hipMemcpyAsync(w.tab, w.h_tab, at_T + (size_t)K * 12 * sizeof(float), hipMemcpyHostToDevice, s));
  int rc = uploads_before_compute(h);
  if (rc) return rc;

  float* X = w.x;
  const McKf* d_kf = (const McKf*)(unsigned char*)w.tab;
  const float* d_T = (const float*)((unsigned char*)w.tab + at_T);
  const int gx = (int)((pitch + 255) / 256);
  k_mc_transform<<<nchunks, MC_THREADS, 0, s>>>(d_kf, K, d_T, (int)n, pitch, X, w.keep, w.aabb);
  k_mc_box<<<1, MC_THREADS, 0, s>>>(X, pitch, w.keep, w.aabb, (int)n, resolution, w.box);
  k_mc_keys<<<gx, 256, 0, s>>>(X, pitch, w.keep, w.box, resolution, w.keys, w.vals);
  // Stable LSD sort of the 64-bit codes with ndt_segsort.hpp's passes: the low words (keys) carrying the high words (vals), then the high
  // words carrying the low words.  The final depth (3 * depth code bits) is only known on the device, so both words are sorted whole
  // (3 + 3 passes of 11 bits): reading it back first would cost a host round trip in the middle of the chain.
  const RsSorted lo = rs_sort_one_segment(s, 32, w.keys, w.vals, w.keys + pitch, w.vals + pitch, pitch, w.hist, w.offs);
  const RsSorted hi = rs_sort_one_segment(s, 32, lo.vals, lo.keys, lo.vals_free, lo.keys_free, pitch, w.hist, w.offs);
  const unsigned *hi_s = hi.keys, *lo_s = hi.vals;
  k_mc_heads<<<gx, 256, 0, s>>>(lo_s, hi_s, pitch, w.flag);
  exscan_ints(s, w.flag, pitch, w.tmp, w.pos);
  k_mc_emit<<<gx, 256, 0, s>>>(lo_s, hi_s, w.flag, w.pos, pitch, w.box, resolution, w.out);
  HIPCHK(h, hipGetLastError());
  int* ret = w.h_ret;                             // status, depth, last scan position, last head flag
  HIPCHK(h, hipMemcpyAsync(ret, &((McBox*)w.box)->status, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(ret + 1, &((McBox*)w.box)->depth, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(ret + 2, w.pos + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(ret + 3, w.flag + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  rc = compute_enqueued(h);                       // later uploads into the staging rows wait for these kernels
  if (rc) return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  w.pending = false;
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
      if (m) HIPCHK(h, hipMemcpy(out_pts, w.out, m * 12, hipMemcpyDeviceToHost));
    } else {
      std::vector<float> tmp(3 * m);
      if (m) HIPCHK(h, hipMemcpy(tmp.data(), w.out, m * 12, hipMemcpyDeviceToHost));
      unsigned char* o = (unsigned char*)out_pts;
      for (size_t i = 0; i < m; i++) memcpy(o + i * out_stride_bytes, &tmp[3 * i], 12);
    }
  }
  return MI355NDT_OK;
}
