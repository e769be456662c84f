// ndt_host_prefilter.hpp -- the prefilter (distance filter + voxel down-sampling) and handing its result to the registration on the device.
#pragma once

// replaces PrefilteringNodelet::distance_filter + downsample (prefiltering_nodelet.cpp:137-181)
int mi355ndt_prefilter(mi355ndt_handle* h, const void* pts, size_t n, size_t stride,
                       int use_distance_filter, double distance_near, double distance_far, float downsample_resolution,
                       void* out_pts, size_t out_capacity, size_t out_stride, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if ((!pts && n) || (n && stride < 12) || n >= (1u << 30) || !n_out || (out_pts && out_stride < 12)) return MI355NDT_ERR_BAD_ARG;
  if (std::isnan(downsample_resolution)) return MI355NDT_ERR_BAD_ARG;
  *n_out = 0;
  h->pf_count = 0;
  if (n == 0) return MI355NDT_OK;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t pitch = (n + 63) & ~(size_t)63;
  if (pitch > h->d_pf_pos.cap) HIPCHK(h, hipStreamSynchronize(s));   // (d_pf_pos grows last: the workspace is re-allocated, nothing may still read it)
  HIPCHK(h, h->d_pf_in.reserve(3 * pitch)); HIPCHK(h, h->d_pf_out.reserve(3 * pitch)); HIPCHK(h, h->d_pf_keep.reserve(pitch));
  HIPCHK(h, h->d_pf_keys.reserve(2 * pitch)); HIPCHK(h, h->d_pf_vals.reserve(2 * pitch)); HIPCHK(h, h->d_pf_flag.reserve(pitch)); HIPCHK(h, h->d_pf_pos.reserve(pitch));
  HIPCHK(h, h->d_pf_mm.reserve(6)); HIPCHK(h, h->d_pf_grid.reserve(1));
  h->pf_pitch = pitch;
  int rc = upload_cloud(h, h->d_pf_in, pitch, 0, pts, n, stride);
  if (rc) return rc;
  rc = uploads_before_compute(h);
  if (rc) return rc;
  const int gx = (int)((pitch + 255) / 256);
  unsigned *ka = h->d_pf_keys, *kb = h->d_pf_keys + pitch, *va = h->d_pf_vals, *vb = h->d_pf_vals + pitch;
  // workspace of the segment sort (one segment = the whole cloud) and of the emit-position scan
  const int pf_tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
  const int pf_chunks = (int)((pitch + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK);
  HIPCHK(h, h->d_rs_hist.reserve((size_t)pf_tiles << RS_MAX_BITS)); HIPCHK(h, h->d_rs_offs.reserve((size_t)pf_tiles << RS_MAX_BITS));
  HIPCHK(h, h->d_pf_tmp.reserve((size_t)pf_chunks));
  k_minmax_init<<<1, 64, 0, s>>>(h->d_pf_mm, 1);
  k_pf_flag<<<std::min(gx, 256), 256, 0, s>>>(h->d_pf_in, pitch, (int)n, use_distance_filter, distance_near, distance_far, h->d_pf_keep, h->d_pf_mm);
  int downsample = downsample_resolution > 0.f;
  const unsigned* keys_sorted = ka;
  const unsigned* vals_sorted = va;
  if (downsample) {
    k_pf_grid<<<1, 1, 0, s>>>(h->d_pf_mm, downsample_resolution, h->d_pf_grid);
    PfGrid g;
    HIPCHK(h, hipMemcpyAsync(&g, h->d_pf_grid, sizeof g, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (g.status == 2) {                         // PCL: "Leaf size is too small for the input dataset" -> output = input
      h->err = "prefilter: leaf size too small for the cloud's extent, voxel indices would overflow; cloud not down-sampled";
      downsample = 0;
    } else {
      k_pf_keys<<<gx, 256, 0, s>>>(h->d_pf_in, pitch, (int)n, h->d_pf_keep, h->d_pf_grid, ka, va);
      // stable sort by voxel index: the target build's segment sort with the whole cloud as its one segment, 31 key bits
      const RsPlan plan = rs_plan(31);
      unsigned *kin = ka, *kout = kb, *vin = va, *vout = vb;
      for (int p = 0; p < plan.passes; p++) {
        rs_pass(s, plan.bits, kin, vin, kout, vout, pitch, p * plan.bits, h->d_rs_hist, h->d_rs_offs, pf_tiles, 1, false);
        std::swap(kin, kout); std::swap(vin, vout);
      }
      keys_sorted = kin; vals_sorted = vin;      // (an odd number of hops ends in kb / vb)
    }
  }
  k_pf_heads<<<gx, 256, 0, s>>>(keys_sorted, h->d_pf_keep, (int)n, pitch, downsample, h->d_pf_flag);
  k_pf_scan_totals<<<pf_chunks, 1024, 0, s>>>(h->d_pf_flag, pitch, h->d_pf_tmp);
  k_pf_scan_offsets<<<1, 1024, 0, s>>>(h->d_pf_tmp, pf_chunks);
  k_pf_scan_apply<<<pf_chunks, 1024, 0, s>>>(h->d_pf_flag, pitch, h->d_pf_tmp, h->d_pf_pos);
  k_pf_emit<<<gx, 256, 0, s>>>(h->d_pf_in, pitch, keys_sorted, vals_sorted, h->d_pf_flag, h->d_pf_pos, downsample, h->d_pf_out, pitch);
  int last_pos = 0, last_flag = 0;
  HIPCHK(h, hipMemcpyAsync(&last_pos, h->d_pf_pos + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(&last_flag, h->d_pf_flag + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  const size_t m = (size_t)last_pos + (size_t)last_flag;
  h->pf_count = (int)m;
  *n_out = m;
  if (out_pts) {
    if (m > out_capacity) return MI355NDT_ERR_BAD_ARG;
    std::vector<float> tmp(3 * pitch);
    HIPCHK(h, hipMemcpy(tmp.data(), h->d_pf_out, 3 * pitch * sizeof(float), hipMemcpyDeviceToHost));
    unsigned char* o = (unsigned char*)out_pts;
    for (size_t i = 0; i < m; i++) {
      float v[3] = {tmp[i], tmp[pitch + i], tmp[2 * pitch + i]};
      memcpy(o + i * out_stride, v, 12);
    }
  }
  return MI355NDT_OK;
}

// hand the last prefilter result to the registration without leaving the GPU: role 1 = setInputSource, 2 = setInputTarget
int mi355ndt_use_prefiltered(mi355ndt_handle* h, int role) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (role != 1 && role != 2) return MI355NDT_ERR_BAD_ARG;
  if (!h->d_pf_out) return MI355NDT_ERR_STATE;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t m = (size_t)h->pf_count;
  int rc = ensure_single(h, role == 2, m);
  if (rc) return rc;
  rc = uploads_before_compute(h);                 // an earlier upload into the same rows must not land after these copies
  if (rc) return rc;
  float* dst = role == 2 ? h->d_tgt_own : h->d_src_own;
  const size_t dp = role == 2 ? h->tgt_pitch : h->src_pitch;
  HIPCHK(h, hipMemsetAsync(dst, 0, 3 * dp * sizeof(float), h->stream));
  for (int a = 0; a < 3; a++)
    if (m) HIPCHK(h, hipMemcpyAsync(dst + a * dp, h->d_pf_out + a * h->pf_pitch, m * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  if (role == 2) {
    h->h_tgt_cnt[0] = (int)m; h->have_target = true; h->targets_built = false;
    return mi355ndt_batch_build_targets(h);
  }
  h->h_src_cnt[0] = (int)m; h->have_source = true;
  return compute_enqueued(h);
}
