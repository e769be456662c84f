// ndt_host_keyframe.hpp -- keyframes that stay on the device: mi355ndt_window_keyframe / _window_keyframe_ids (the window map -> keyframe cloud,
// over host scans or resident ones), the keyframe store (mi355ndt_keyframe_add / _get / _release / _count, mi355ndt_keyframe_from_prefiltered /
// _from_slot) and the consumers that take ids (mi355ndt_map_cloud_keyframes,
// mi355ndt_batch_set_target_keyframe / _source_keyframe).  The batch, the grids, the prefilter result and the store's other keyframes are left
// as they were; the window map's scratch is the shared one (h->vs).
#pragma once

static mi355ndt_handle::Keyframe* kf_find(mi355ndt_handle* h, int id, const char* where) {
  auto it = h->keyframes.find(id);
  if (it == h->keyframes.end()) {
    h->err = std::string(where) + ": no keyframe with id " + std::to_string(id) + (id >= 0 && id < h->kf_next_id ? " (released)" : " (never given out)");
    return nullptr;
  }
  return &it->second;
}

// rows for a keyframe of m points with `ch` channels; an empty keyframe owns nothing
static int kf_alloc(mi355ndt_handle* h, mi355ndt_handle::Keyframe& kf, size_t m, int ch) {
  kf.n = m; kf.ch = ch; kf.pitch = (m + 63) & ~(size_t)63;
  if (kf.pitch) HIPCHK(h, kf.rows.realloc_exact((size_t)ch * kf.pitch));
  return MI355NDT_OK;
}

// ---- window map -> keyframe ------------------------------------------------------------------------
// replaces the window accumulation and down-sampling of GlobalGraphNodelet::cloud_callback (global_graph_nodelet.cpp:202-244).  Between its
// own flag pass (k_kf_window) and its own emit the window is the prefilter chain's one cloud (pfb_positions).  The scans are host records
// (mi355ndt_window_keyframe: they go up through the engine's staging as the map cloud's keyframes do) or resident keyframes
// (mi355ndt_window_keyframe_ids: the scan table points into the store, nothing is staged); everything else is one body.  The call waits for
// the device once -- for the count, which sizes the keyframe's rows -- and returns with the emit kernel enqueued.
struct KfWindow {
  int K, ch; size_t n, pitch, at_tab, at_item; float leaf;
  double* T; KfScan* tab;                          // the pinned twins of the poses and the scan table, for the caller to fill
};
// the window's scratch and tables for K scans of n points in all (n > 0); in_floats: what the staged scans need of `in`
static int kf_window_begin(mi355ndt_handle* h, int K, size_t n, int ch, float leaf, size_t in_floats, const double* rel_poses, KfWindow* win) {
  VoxelScratch& w = h->vs;
  win->K = K; win->ch = ch; win->n = n; win->leaf = leaf;
  win->pitch = (n + 63) & ~(size_t)63;
  win->at_tab = (size_t)K * 12 * sizeof(double); win->at_item = win->at_tab + (size_t)K * sizeof(KfScan);
  static_assert(sizeof(KfScan) % 8 == 0, "the tables' layout");
  VsNeed need;
  need.pitch = win->pitch; need.in = in_floats; need.x = (size_t)ch * win->pitch; need.tab = win->at_item + sizeof(PfbItem); need.stat = PFB_RES_WORDS(1);
  const int rc = vs_reserve(h, need);              // (an earlier window's emit kernel may still run: it is waited for if anything grows)
  if (rc) return rc;
  // poses ((w_odom.inverse() * odom_k).matrix(), column-major f64 -> row-major rows 0..2), scan table and the chain's item (nothing is emitted
  // through it: a pitch no count exceeds), one pinned block, one copy
  win->T = (double*)(unsigned char*)w.h_tab;
  win->tab = (KfScan*)((unsigned char*)w.h_tab + win->at_tab);
  *(PfbItem*)((unsigned char*)w.h_tab + win->at_item) = PfbItem{nullptr, ~0ull, (int)n, 0};
  for (int k = 0; k < K; k++)
    for (int a = 0; a < 3; a++)
      for (int j = 0; j < 4; j++) win->T[12 * k + 4 * a + j] = k == 0 ? (a == j ? 1.0 : 0.0) : rel_poses[16 * k + 4 * j + a];   // (scan 0 is not moved)
  return MI355NDT_OK;
}
// the tables go down, the chain runs over the scans the table names, and the window becomes keyframe *id.  (The caller has ordered whatever
// fills the scans' rows before the compute stream: uploads_before_compute.)
static int kf_window_finish(mi355ndt_handle* h, const KfWindow& win, int* id, size_t* n_out) {
  hipStream_t s = h->stream;
  VoxelScratch& w = h->vs;
  const size_t pitch = win.pitch;
  const int nblk = (int)((pitch + KF_CHUNK - 1) / KF_CHUNK), ch = win.ch;
  PfbChain chain;                                 // the window as the prefilter chain's one cloud: no gate, VOXELGRID
  memset(&chain, 0, sizeof chain);
  chain.leaf = win.leaf; chain.downsample = win.leaf > 0.f; chain.ioff = -1;
  w.pending = true;
  HIPCHK(h, hipMemcpyAsync(w.tab, w.h_tab, win.at_item + sizeof(PfbItem), hipMemcpyHostToDevice, s));
  float* X = w.x;
  const int gx = (int)((pitch + 255) / 256);
  const PfbItem* item = (const PfbItem*)((unsigned char*)w.tab + win.at_item);
  k_pfb_begin<<<1, 256, 0, s>>>(w.mm, w.stat, 1);
  k_kf_window<<<nblk, KF_THREADS, 0, s>>>((const KfScan*)((unsigned char*)w.tab + win.at_tab), win.K, (const double*)(unsigned char*)w.tab, (int)win.n, pitch, ch, X, w.keep, w.mm);
  const PfbSorted v = pfb_positions(s, w, chain, X, item, 1, pitch);
  HIPCHK(h, hipGetLastError());
  int* ret = w.h_ret;                             // the count, the overflow word (never raised), the too-small word
  HIPCHK(h, hipMemcpyAsync(ret, w.stat, PFB_RES_WORDS(1) * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  w.pending = false;
  const size_t m = (size_t)ret[0];
  if (ret[2] != INT_MAX) h->err = "window_keyframe: leaf size too small for the window's extent, voxel indices would overflow; window not down-sampled";
  mi355ndt_handle::Keyframe kf;
  const int rc = kf_alloc(h, kf, m, ch);
  if (rc) return rc;
  if (m) {
    k_kf_emit<<<gx, 256, 0, s>>>(X, pitch, v.keys, v.vals, w.flag, w.pos, w.grid, chain.downsample, ch, kf.rows, kf.pitch, m);
    HIPCHK(h, hipGetLastError());
  }
  *id = h->kf_next_id++;
  *n_out = m;
  h->keyframes.emplace(*id, std::move(kf));
  return MI355NDT_OK;
}
// a keyframe without a point (a window without one, an empty resident cloud): it owns nothing
static int kf_store_empty(mi355ndt_handle* h, int ch, int* id) {
  mi355ndt_handle::Keyframe kf;
  kf_alloc(h, kf, 0, ch);
  *id = h->kf_next_id++;
  h->keyframes.emplace(*id, std::move(kf));
  return MI355NDT_OK;
}

int mi355ndt_window_keyframe(mi355ndt_handle* h, int n_scans, const void* const* scans, const size_t* counts, size_t stride_bytes,
                             int intensity_offset_bytes, const double* rel_poses, float leaf, int* id, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!id || !n_out || n_scans <= 0 || !scans || !counts || (n_scans > 1 && !rel_poses) || std::isnan(leaf)) return MI355NDT_ERR_BAD_ARG;
  *id = -1; *n_out = 0;
  const int K = n_scans, ioff = intensity_offset_bytes, ch = ioff >= 0 ? 4 : 3;
  size_t n = 0, in_total = 0;
  for (int k = 0; k < K; k++) {
    if (counts[k] && (!scans[k] || stride_bytes < 12 || (ioff >= 0 && (size_t)ioff + 4 > stride_bytes))) return MI355NDT_ERR_BAD_ARG;
    n += counts[k];
    in_total += (size_t)ch * ((counts[k] + 63) & ~(size_t)63);
    if (n >= (1u << 30)) return MI355NDT_ERR_BAD_ARG;   // (the prefilter's limit: int positions, 32-bit scan)
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (n == 0) return kf_store_empty(h, ch, id);   // a window without a point: an empty keyframe
  KfWindow win;
  int rc = kf_window_begin(h, K, n, ch, leaf, in_total, rel_poses, &win);
  if (rc) return rc;
  VoxelScratch& w = h->vs;
  std::vector<UpItem> items;
  items.reserve((size_t)K);
  size_t start = 0, base = 0;
  for (int k = 0; k < K; k++) {
    const size_t kp = (counts[k] + 63) & ~(size_t)63;
    win.tab[k] = KfScan{w.in + base, (unsigned)start, (unsigned)kp, ch == 4 ? w.in + base + 3 * kp : nullptr};
    if (counts[k]) items.push_back(UpItem{w.in + base, kp, 0, scans[k], counts[k], stride_bytes, ioff});
    start += counts[k]; base += (size_t)ch * kp;
  }
  rc = upload_items_grouped(h, items);
  if (rc) return rc;
  rc = uploads_before_compute(h);
  if (rc) return rc;
  return kf_window_finish(h, win, id, n_out);
}

// the same over resident scans: scan k is keyframe ids[k] as it is stored
int mi355ndt_window_keyframe_ids(mi355ndt_handle* h, int n_scans, const int* ids, const double* rel_poses, float leaf, int with_intensity,
                                 int* id, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!id || !n_out || n_scans <= 0 || !ids || (n_scans > 1 && !rel_poses) || std::isnan(leaf)) return MI355NDT_ERR_BAD_ARG;
  *id = -1; *n_out = 0;
  const int K = n_scans, ch = with_intensity ? 4 : 3;
  size_t n = 0;
  for (int k = 0; k < K; k++) {
    const mi355ndt_handle::Keyframe* kf = kf_find(h, ids[k], "window_keyframe_ids");
    if (!kf) return MI355NDT_ERR_BAD_ARG;
    n += kf->n;
    if (n >= (1u << 30)) return MI355NDT_ERR_BAD_ARG;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (n == 0) return kf_store_empty(h, ch, id);
  KfWindow win;
  int rc = kf_window_begin(h, K, n, ch, leaf, 0, rel_poses, &win);
  if (rc) return rc;
  size_t start = 0;
  for (int k = 0; k < K; k++) {
    const mi355ndt_handle::Keyframe& kf = h->keyframes.find(ids[k])->second;
    win.tab[k] = KfScan{kf.rows, (unsigned)start, (unsigned)kf.pitch, kf.ch == 4 && kf.n ? kf.rows + 3 * kf.pitch : nullptr};
    start += kf.n;
  }
  rc = uploads_before_compute(h);                 // (a mi355ndt_keyframe_add's transfer into a scan may still be on its way)
  if (rc) return rc;
  return kf_window_finish(h, win, id, n_out);
}

// ---- resident scans into the store -------------------------------------------------------------------
// m points of device rows (x, y, z at rows + a * src_pitch; irow: the intensity row or null) into a new keyframe of 3 or 4 channels, device to
// device on the engine's stream: the keyframe owns its rows (pitch rounded to 64, tail zeroed) and the source is left as it was
static int kf_from_rows(mi355ndt_handle* h, const float* rows, size_t src_pitch, const float* irow, size_t m, int* id) {
  const int ch = irow ? 4 : 3;
  if (m == 0) return kf_store_empty(h, ch, id);
  mi355ndt_handle::Keyframe kf;
  int rc = kf_alloc(h, kf, m, ch);
  if (rc) return rc;
  rc = uploads_before_compute(h);                 // pending uploads into the source land first (kernels into it run on this stream)
  if (rc) return rc;
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemsetAsync(kf.rows, 0, (size_t)ch * kf.pitch * sizeof(float), s));
  for (int a = 0; a < 3; a++) HIPCHK(h, hipMemcpyAsync(kf.rows + (size_t)a * kf.pitch, rows + (size_t)a * src_pitch, m * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (irow) HIPCHK(h, hipMemcpyAsync(kf.rows + 3 * kf.pitch, irow, m * sizeof(float), hipMemcpyDeviceToDevice, s));
  rc = compute_enqueued(h);                       // a later upload into the source waits for the copies
  if (rc) return rc;
  *id = h->kf_next_id++;
  h->keyframes.emplace(*id, std::move(kf));
  return MI355NDT_OK;
}
int mi355ndt_keyframe_from_prefiltered(mi355ndt_handle* h, int* id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!id) return MI355NDT_ERR_BAD_ARG;
  *id = -1;
  if (!h->pf_resident) { h->err = "keyframe_from_prefiltered: no prefilter result is resident (mi355ndt_prefilter first)"; return MI355NDT_ERR_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  const size_t m = (size_t)h->pf_count;
  if (m == 0) return kf_store_empty(h, h->pf_ch, id);
  return kf_from_rows(h, h->d_pf_out, h->pf_pitch, h->pf_ch == 4 ? h->d_pf_out + 3 * h->pf_pitch : nullptr, m, id);
}
int mi355ndt_keyframe_from_slot(mi355ndt_handle* h, int pair, int role, int* id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!id || pair < 0 || pair >= h->n_pairs || (role != 1 && role != 2)) return MI355NDT_ERR_BAD_ARG;
  *id = -1;
  const bool tgt = role == 2;
  if (!(tgt ? h->have_target : h->have_source)) { h->err = "keyframe_from_slot: a side that has never been given a cloud"; return MI355NDT_ERR_BAD_ARG; }
  const float* base = tgt ? h->d_tgt : h->d_src;
  if (!base) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t pitch = tgt ? h->tgt_pitch : h->src_pitch;
  const size_t m = (size_t)(tgt ? h->h_tgt_cnt : h->h_src_cnt)[(size_t)pair];
  const float* irow = slot_intensity_row(h, tgt, pair);
  if (m == 0) return kf_store_empty(h, irow ? 4 : 3, id);
  return kf_from_rows(h, base + (size_t)pair * 3 * pitch, pitch, irow, m, id);
}

// ---- keyframe store ---------------------------------------------------------------------------------
// a host cloud as it is (x, y, z and, with intensity_offset_bytes >= 0, the f32 at that offset of every record)
int mi355ndt_keyframe_add(mi355ndt_handle* h, const void* pts, size_t n, size_t stride_bytes, int intensity_offset_bytes, int* id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  const int ioff = intensity_offset_bytes, ch = ioff >= 0 ? 4 : 3;
  if (!id || (n && (!pts || stride_bytes < 12 || (ioff >= 0 && (size_t)ioff + 4 > stride_bytes))) || n >= (1u << 30)) return MI355NDT_ERR_BAD_ARG;
  *id = -1;
  HIPCHK(h, hipSetDevice(h->device));
  mi355ndt_handle::Keyframe kf;
  int rc = kf_alloc(h, kf, n, ch);
  if (rc) return rc;
  if (n) {
    const UpItem it = {kf.rows, kf.pitch, 0, pts, n, stride_bytes, ioff};
    rc = upload_items(h, &it, 1);
    if (rc) {                                     // (the rows go away with kf: nothing of a transfer may still be under way into them)
      for (hipStream_t cs : h->copy_stream) (void)hipStreamSynchronize(cs);
      return rc;
    }
  }
  *id = h->kf_next_id++;
  h->keyframes.emplace(*id, std::move(kf));
  return MI355NDT_OK;
}

int mi355ndt_keyframe_get(mi355ndt_handle* h, int id, void* out_pts, size_t out_capacity, size_t out_stride_bytes, int out_intensity_offset_bytes,
                          size_t* n) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!n) return MI355NDT_ERR_BAD_ARG;
  *n = 0;
  const mi355ndt_handle::Keyframe* kf = kf_find(h, id, "keyframe_get");
  if (!kf) return MI355NDT_ERR_BAD_ARG;
  *n = kf->n;
  if (!out_pts || kf->n == 0) return MI355NDT_OK;
  const int ioff = out_intensity_offset_bytes;
  if (out_stride_bytes < 12 || (ioff >= 0 && (size_t)ioff + 4 > out_stride_bytes) || kf->n > out_capacity) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = uploads_before_compute(h);             // (a keyframe_add's transfer may still be on its way)
  if (rc) return rc;
  std::vector<float> tmp((size_t)kf->ch * kf->pitch);
  HIPCHK(h, hipMemcpyAsync(tmp.data(), kf->rows, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  rows_to_records(tmp.data(), kf->pitch, kf->ch, kf->n, out_pts, out_stride_bytes, ioff);
  return MI355NDT_OK;
}

int mi355ndt_keyframe_release(mi355ndt_handle* h, int id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!kf_find(h, id, "keyframe_release")) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));   // nothing enqueued may still read or fill the rows
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->vs.pending = false;
  h->keyframes.erase(id);
  return MI355NDT_OK;
}

int mi355ndt_keyframe_count(const mi355ndt_handle* h) { return !h ? MI355NDT_ERR_BAD_HANDLE : h->ss ? MI355NDT_ERR_STATE : (int)h->keyframes.size(); }

// ---- consumers by id -------------------------------------------------------------------------------
// mi355ndt_map_cloud over resident keyframes: the McKf table points into the store, nothing is staged
int mi355ndt_map_cloud_keyframes(mi355ndt_handle* h, int n_keyframes, const int* ids, const double* poses, double resolution,
                                 void* out_pts, size_t out_capacity, size_t out_stride_bytes, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (!n_out || n_keyframes < 0 || (out_pts && out_stride_bytes < 12)) return MI355NDT_ERR_BAD_ARG;
  *n_out = 0;
  if (n_keyframes == 0) return MI355NDT_OK;
  if (!(resolution > 0) || !std::isfinite(resolution) || !ids || !poses) return MI355NDT_ERR_BAD_ARG;
  const int K = n_keyframes;
  size_t n = 0;
  for (int k = 0; k < K; k++) {
    const mi355ndt_handle::Keyframe* kf = kf_find(h, ids[k], "map_cloud_keyframes");
    if (!kf) return MI355NDT_ERR_BAD_ARG;
    n += kf->n;
    if (n >= (1u << 30)) return MI355NDT_ERR_BAD_ARG;
  }
  if (n == 0) return MI355NDT_OK;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = mc_reserve(h, K, n, 0);
  if (rc) return rc;
  McKf* tab = (McKf*)(unsigned char*)h->vs.h_tab;
  size_t start = 0;
  for (int k = 0; k < K; k++) {
    const mi355ndt_handle::Keyframe& kf = h->keyframes.find(ids[k])->second;
    tab[k].rows = kf.rows; tab[k].start = (unsigned)start; tab[k].pitch = (unsigned)kf.pitch;
    start += kf.n;
  }
  return mc_generate(h, K, n, poses, resolution, out_pts, out_capacity, out_stride_bytes, n_out);
}

// A resident keyframe into a slot of the engine's own batch rows, device to device: what mi355ndt_batch_set_target / _source do with a host
// cloud (the slot's rows zero-filled up to the pitch).
static int batch_set_side_keyframe(mi355ndt_handle* h, bool tgt, int pair, int id) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (pair < 0 || pair >= h->n_pairs || (tgt ? h->d_tgt != h->d_tgt_own : h->d_src != h->d_src_own)) return MI355NDT_ERR_BAD_ARG;
  const mi355ndt_handle::Keyframe* kf = kf_find(h, id, tgt ? "batch_set_target_keyframe" : "batch_set_source_keyframe");
  if (!kf) return MI355NDT_ERR_BAD_ARG;
  const size_t dp = tgt ? h->tgt_pitch : h->src_pitch;
  if (kf->n > dp) { h->err = "batch_set_*_keyframe: the keyframe has more points than mi355ndt_batch_reserve made room for"; return MI355NDT_ERR_BAD_ARG; }
  HIPCHK(h, hipSetDevice(h->device));
  const int rc = rows_into_slot(h, tgt, pair, kf->rows, kf->pitch, kf->n);
  return rc ? rc : compute_enqueued(h);                    // a later upload into these rows waits for the copies
}
int mi355ndt_batch_set_target_keyframe(mi355ndt_handle* h, int pair, int id) { return batch_set_side_keyframe(h, true, pair, id); }
int mi355ndt_batch_set_source_keyframe(mi355ndt_handle* h, int pair, int id) { return batch_set_side_keyframe(h, false, pair, id); }
