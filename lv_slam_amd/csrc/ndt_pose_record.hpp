// ndt_pose_record.hpp -- pose records for the multi-GPU gather: 96 bytes = {float final[16] column-major; float score;
// int iterations; int converged; int pair_id; int pad[4]} per pair, packed on the device -- by k_pose_records from the results of the
// last batch align, or by the one-launch align's updater as it finalises a pair (ndt_async.hpp).
// Rows past the batch (a rank that owns one pair fewer than its neighbours) carry pair_id = -1.
#pragma once
#include "ndt_types.hpp"

struct PoseRecord { float final_cm[16]; float score; int iterations, converged, pair_id, pad[4]; };

__device__ __forceinline__ PoseRecord pose_record_padding() {
  PoseRecord r;
  memset(&r, 0, sizeof r);
  r.pair_id = -1;
  return r;
}
__device__ __forceinline__ PoseRecord pose_record(const float final_cm[16], const double score, const int iterations, const int converged, const int pair_id) {
  PoseRecord r = pose_record_padding();
  for (int a = 0; a < 16; a++) r.final_cm[a] = final_cm[a];
  r.score = (float)score;
  r.iterations = iterations;
  r.converged = converged;
  r.pair_id = pair_id;
  return r;
}

NDT_KERNEL void k_pose_records(const mi355ndt_result* __restrict__ res, int n_pairs, int id_base, int id_stride, PoseRecord* out, int capacity) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= capacity) return;
  out[k] = k < n_pairs ? pose_record(res[k].final_colmajor, res[k].score, res[k].iterations, res[k].converged, id_base + k * id_stride) : pose_record_padding();
}
