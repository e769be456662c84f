// ndt_upload.hpp -- the kernels that move clouds between the caller's layout and the engine's: host clouds arrive as packed records and
// become SoA rows (k_deinterleave, k_deinterleave_multi; the host side is ndt_host_upload.hpp), the aligned cloud goes back as packed
// triples (k_transform).
#pragma once
#include "ndt_types.hpp"

// output cloud of align(): source moved by final_transformation_ (f32), written as packed x,y,z triples (what goes back over PCIe)
NDT_KERNEL void k_transform(const float* __restrict__ src, size_t pitch, const PairState* __restrict__ st, int b, float* out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* X = src + (size_t)b * 3 * pitch;
  const float* F = st[b].final_cm;
  float px = X[i], py = X[pitch + i], pz = X[2 * pitch + i];
  for (int a = 0; a < 3; a++) out[(size_t)3 * i + a] = ((F[0 * 4 + a] * px + F[1 * 4 + a] * py) + F[2 * 4 + a] * pz) + F[3 * 4 + a];
}

// host clouds arrive as packed x,y,z triples (the engine drops the other fields of the caller's records while it stages them in
// pinned memory); this turns one cloud into the SoA rows the kernels read, zero-filling the padding up to the row pitch
NDT_KERNEL void __launch_bounds__(256) k_deinterleave(const float* __restrict__ xyz, int n, float* rows, size_t pitch) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pitch) return;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < (size_t)n) { x = xyz[3 * i]; y = xyz[3 * i + 1]; z = xyz[3 * i + 2]; }
  rows[i] = x; rows[pitch + i] = y; rows[2 * pitch + i] = z;
}

// ... and several clouds of one transfer at once (grid.y = cloud): ndt_host_upload.hpp, upload_items.  A cloud staged with its intensity (w4: four
// words per record) fills a fourth row -- row4: behind the three (a keyframe's, a window scan's) or wherever the host says (the prefilter's
// intensity plane lies beside its [cloud][3][rp] rows) --; the others are read and written exactly as before.
struct DeintTab { int cnt, pad_; struct { unsigned long long src_off; float* rows; unsigned long long pitch; int n, w4; float* row4; } e[16]; };
NDT_KERNEL void __launch_bounds__(256) k_deinterleave_multi(const float* __restrict__ packed, const DeintTab tab) {
  const int c = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t pitch = tab.e[c].pitch;
  if (i >= pitch) return;
  const float* xyz = packed + tab.e[c].src_off;
  float* rows = tab.e[c].rows;
  float x = 0.f, y = 0.f, z = 0.f;
  if (tab.e[c].w4) {
    float w = 0.f;
    if (i < (size_t)tab.e[c].n) { const float4 r = *(const float4*)(xyz + 4 * i); x = r.x; y = r.y; z = r.z; w = r.w; }
    tab.e[c].row4[i] = w;
  } else if (i < (size_t)tab.e[c].n) { x = xyz[3 * i]; y = xyz[3 * i + 1]; z = xyz[3 * i + 2]; }
  rows[i] = x; rows[pitch + i] = y; rows[2 * pitch + i] = z;
}
