// ndt_host_prefilter.hpp -- the prefilter (distance filter + voxel down-sampling) and handing its result to the registration on the device.
// The result (d_pf_out) is the prefilter's own and stays until the next prefilter call; everything before it is the shared scratch (h->vs).
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
  VoxelScratch& w = h->vs;
  VsNeed need;
  need.pitch = pitch; need.in = 3 * pitch;
  int rc = vs_reserve(h, need);
  if (rc) return rc;
  if (3 * pitch > h->d_pf_out.cap) HIPCHK(h, hipStreamSynchronize(s));   // (the result buffer is re-allocated: no copy out of it may still run)
  HIPCHK(h, h->d_pf_out.reserve(3 * pitch));
  h->pf_pitch = pitch;
  rc = upload_cloud(h, w.in, pitch, 0, pts, n, stride);
  if (rc) return rc;
  rc = uploads_before_compute(h);
  if (rc) return rc;
  const int gx = (int)((pitch + 255) / 256);
  k_minmax_init<<<1, 64, 0, s>>>(w.mm, 1);
  k_pf_flag<<<std::min(gx, 256), 256, 0, s>>>(w.in, pitch, (int)n, use_distance_filter, distance_near, distance_far, w.keep, w.mm);
  VgHeads v;
  rc = voxel_grid_heads(h, "prefilter", "cloud", w.in, pitch, n, downsample_resolution, &v);
  if (rc) return rc;
  k_pf_emit<<<gx, 256, 0, s>>>(w.in, pitch, v.keys, v.vals, w.flag, w.pos, v.downsample, h->d_pf_out, pitch);
  int last_pos = 0, last_flag = 0;
  HIPCHK(h, hipMemcpyAsync(&last_pos, w.pos + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(&last_flag, w.flag + (pitch - 1), sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  HIPCHK(h, hipGetLastError());
  const size_t m = (size_t)last_pos + (size_t)last_flag;
  h->pf_count = (int)m;
  *n_out = m;
  if (out_pts) {
    if (m > out_capacity) return MI355NDT_ERR_BAD_ARG;
    std::vector<float> tmp(3 * pitch);
    HIPCHK(h, hipMemcpy(tmp.data(), h->d_pf_out, 3 * pitch * sizeof(float), hipMemcpyDeviceToHost));
    rows_to_records(tmp.data(), pitch, 3, m, out_pts, out_stride, -1);
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
  rc = rows_into_slot(h, role == 2, 0, h->d_pf_out, h->pf_pitch, m);
  if (rc) return rc;
  return role == 2 ? mi355ndt_batch_build_targets(h) : compute_enqueued(h);
}
