// ndt_host_voxel.hpp -- what the prefilter, the map cloud, the window map and the keyframe index builds share on the host: growth of their one
// scratch (VoxelScratch, ndt_engine.hpp), the exclusive scan and the scatter of SoA rows into the caller's records.  (The VoxelGrid chain
// itself is pfb_positions, ndt_host_prefilter.hpp: one segmented chain for one cloud as for K.)
#pragma once

// what a call needs of the scratch: points (a multiple of 64: every per-point member follows from it), floats of in / x / out, bytes of the
// tables, doubles of the partials, status ints; clouds: the segments `pitch` is divided into (the batch prefilter: extremes and a grid per
// cloud, sort tiles and scan chunks per cloud)
struct VsNeed { size_t pitch = 0, in = 0, x = 0, out = 0, tab = 0, part = 0, stat = 0, clouds = 1; };

// The growth rule, once: a member that grows is freed first, so nothing enqueued -- on the copy streams or the compute stream -- may still
// use the scratch.  pos is reserved last: a failed allocation leaves its capacity vouching for nothing that was freed.
static int vs_reserve(mi355ndt_handle* h, const VsNeed& n) {
  VoxelScratch& w = h->vs;
  hipStream_t s = h->stream;
  if (w.pending) { HIPCHK(h, hipStreamSynchronize(s)); w.pending = false; }   // (the host is about to write h_tab)
  // (a cloud's tiles are its own: K clouds of one point past a tile are 2 K tiles)
  const size_t tiles = std::max((n.pitch + RS_TILE - 1) / RS_TILE, n.clouds * ((n.pitch / n.clouds + RS_TILE - 1) / RS_TILE));
  if (n.pitch > w.pos.cap || n.in > w.in.cap || n.x > w.x.cap || n.out > w.out.cap || n.tab > w.tab.cap || n.part > w.part.cap || n.stat > w.stat.cap ||
      (tiles << RS_MAX_BITS) > w.hist.cap || 6 * n.clouds > w.mm.cap) {
    for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));
    HIPCHK(h, hipStreamSynchronize(s));
  }
  HIPCHK(h, w.in.reserve(n.in)); HIPCHK(h, w.x.reserve(n.x)); HIPCHK(h, w.out.reserve(n.out)); HIPCHK(h, w.keep.reserve(n.pitch));
  HIPCHK(h, w.keys.reserve(2 * n.pitch)); HIPCHK(h, w.vals.reserve(2 * n.pitch)); HIPCHK(h, w.flag.reserve(n.pitch));
  HIPCHK(h, w.hist.reserve(tiles << RS_MAX_BITS)); HIPCHK(h, w.offs.reserve(tiles << RS_MAX_BITS));
  HIPCHK(h, w.tmp.reserve(std::max((n.pitch + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK, tiles))); HIPCHK(h, w.aabb.reserve(6 * ((n.pitch + MC_CHUNK - 1) / MC_CHUNK)));
  HIPCHK(h, w.mm.reserve(6 * n.clouds)); HIPCHK(h, w.cnt.reserve(1)); HIPCHK(h, w.grid.reserve(n.clouds)); HIPCHK(h, w.box.reserve(1));
  HIPCHK(h, w.tab.reserve(n.tab)); HIPCHK(h, w.h_tab.reserve(n.tab)); HIPCHK(h, w.part.reserve(n.part)); HIPCHK(h, w.h_part.reserve(n.part));
  HIPCHK(h, w.stat.reserve(n.stat)); HIPCHK(h, w.h_ret.reserve(std::max((size_t)4, n.stat)));
  HIPCHK(h, w.pos.reserve(n.pitch));
  return MI355NDT_OK;
}

// exclusive scan of `pitch` ints (ndt_prefilter.hpp); tmp: one word per PF_SCAN_CHUNK
static void exscan_ints(hipStream_t s, const int* flag, size_t pitch, unsigned* tmp, int* pos) {
  const int chunks = (int)((pitch + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK);
  k_pf_scan_totals<<<chunks, 1024, 0, s>>>(flag, pitch, tmp);
  k_pf_scan_offsets<<<1, 1024, 0, s>>>(tmp, chunks);
  k_pf_scan_apply<<<chunks, 1024, 0, s>>>(flag, pitch, tmp, pos);
}

// n points of host SoA rows (`ch` rows of `pitch` floats: x, y, z and, with ch = 4, the intensity) into the caller's records; ioff >= 0: the
// record's f32 at that byte offset receives the intensity (0 where the rows carry none)
static void rows_to_records(const float* rows, size_t pitch, int ch, size_t n, void* out_pts, size_t out_stride, int ioff) {
  unsigned char* o = (unsigned char*)out_pts;
  for (size_t i = 0; i < n; i++) {
    const float v[3] = {rows[i], rows[pitch + i], rows[2 * pitch + i]};
    memcpy(o + i * out_stride, v, 12);
    if (ioff >= 0) { const float w = ch == 4 ? rows[3 * pitch + i] : 0.f; memcpy(o + i * out_stride + ioff, &w, 4); }
  }
}
