// ndt_host_prefilter.hpp -- the prefilter (distance filter + voxel down-sampling) and handing its result to the registration on the device.
// The result (d_pf_out) is the prefilter's own and stays until the next prefilter call; everything before it is the shared scratch (h->vs).
#pragma once

// the first m points of the resident result into the caller's records (out_pts may be null: nothing is fetched); a result with an intensity
// row writes it at the offset it had in the input records (the callers have checked that out_stride holds it)
static int pf_result_records(mi355ndt_handle* h, size_t m, void* out_pts, size_t out_capacity, size_t out_stride) {
  if (!out_pts) return MI355NDT_OK;
  if (m > out_capacity) return MI355NDT_ERR_BAD_ARG;
  const size_t pitch = h->pf_pitch;
  const int ch = h->pf_ch;
  std::vector<float> tmp((size_t)ch * pitch);
  HIPCHK(h, hipMemcpy(tmp.data(), h->d_pf_out, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
  rows_to_records(tmp.data(), pitch, ch, m, out_pts, out_stride, ch == 4 ? h->pf_ioff : -1);
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

// ---- whole batches of raw scans into the batch slots (ndt_prefilter_batch.hpp) -------------------------------------------------------------
int mi355ndt_prefilter_params_default(mi355ndt_prefilter_params* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  memset(p, 0, sizeof *p);
  p->use_distance_filter = 1; p->distance_near = 1.0; p->distance_far = 100.0;   // prefiltering_nodelet.cpp:83-85
  p->downsample_resolution = 0.1f;
  for (int a = 0; a < 4; a++) p->transform_colmajor[5 * a] = 1.f;
  return MI355NDT_OK;
}
int mi355ndt_prefilter_params_ex_default(mi355ndt_prefilter_params_ex* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  memset(p, 0, sizeof *p);
  (void)mi355ndt_prefilter_params_default(&p->base);
  p->base.extended = MI355NDT_PREFILTER_EXTENDED;
  p->downsample_method = MI355NDT_DOWNSAMPLE_VOXELGRID;
  p->use_angle_calibration = 0; p->angle_calibration_rad = 0.11 * M_PI / 180;      // :88, :190
  return MI355NDT_OK;
}
int mi355ndt_prefilter_params_ex2_default(mi355ndt_prefilter_params_ex2* p) {
  if (!p) return MI355NDT_ERR_BAD_ARG;
  memset(p, 0, sizeof *p);
  (void)mi355ndt_prefilter_params_ex_default(&p->ex);
  p->ex.base.extended = MI355NDT_PREFILTER_EXTENDED2;
  p->intensity_offset_bytes = -1;
  return MI355NDT_OK;
}

// The scratch of a group of K raw clouds of pitch rp, per raw point: rows 12 B + keep 1 + two key and two id arrays (sort ping-pong) 16 + flag 4
// + pos 4 + the sort's tile histograms and offsets 2 x (2048 words per 4096-point tile) = 4: 41 B (with the intensity plane: 45).  Groups are cut so that K * rp * 41 stays
// under 2 GiB: 399 clouds of 131,072 points, 52 M raw points, whatever their number in the call.  (At most PFB_GROUP_MAX clouds: the per-cloud
// words stay small beside the per-point ones.)  APPROX_VOXELGRID uses the same arrays; what it needs on top -- 512 bucket words per cloud
// behind the flags and the positions -- is in its pitch (pfb_pitch), so the same 41 B per position size its groups.
#define PFB_POINT_BYTES    41
#define PFB_SCRATCH_BUDGET ((size_t)2 << 30)
#define PFB_GROUP_MAX      4096

// What a prefilter chain does to every cloud of a group, decided once per call from the nodelet's parameters.
struct PfbChain {
  int use_df; double dnear, dfar;
  float leaf; int downsample, approx;              // downsample: leaf > 0; approx: APPROX_VOXELGRID and downsample
  PfbMove mv; PfCal cal;
  int ioff;                                        // byte offset of the records' intensity (< 0: none; mi355ndt_prefilter_params_ex2)
};
// From the caller's parameters (NULL: the defaults; a mi355ndt_prefilter_params, or the base of a mi355ndt_prefilter_params_ex / _ex2 when it
// says so): every parameter a call refuses, before anything is staged.  stride: of the call's records when it has any point (else 0: the
// intensity's offset is not held against it).
static int pfb_chain(const mi355ndt_prefilter_params* prm, size_t stride, PfbChain* c) {
  mi355ndt_prefilter_params_ex x;
  (void)mi355ndt_prefilter_params_ex_default(&x);
  int ioff = -1;
  if (prm && prm->extended == MI355NDT_PREFILTER_EXTENDED2) {
    const mi355ndt_prefilter_params_ex2& x2 = *(const mi355ndt_prefilter_params_ex2*)prm;
    x = x2.ex;
    ioff = x2.intensity_offset_bytes < 0 ? -1 : x2.intensity_offset_bytes;
    if (x2.reserved != 0) return MI355NDT_ERR_BAD_ARG;
    if (ioff >= 0 && (ioff < 12 || ioff % 4 != 0 || (stride && (size_t)ioff + 4 > stride))) return MI355NDT_ERR_BAD_ARG;
  } else if (prm && prm->extended == MI355NDT_PREFILTER_EXTENDED) x = *(const mi355ndt_prefilter_params_ex*)prm;
  else if (prm) x.base = *prm;
  const mi355ndt_prefilter_params& p = x.base;
  if (std::isnan(p.downsample_resolution)) return MI355NDT_ERR_BAD_ARG;
  if (p.use_transform) for (float v : p.transform_colmajor) if (std::isnan(v)) return MI355NDT_ERR_BAD_ARG;
  if (x.downsample_method != MI355NDT_DOWNSAMPLE_VOXELGRID && x.downsample_method != MI355NDT_DOWNSAMPLE_APPROX_VOXELGRID) return MI355NDT_ERR_BAD_ARG;
  if (!std::isfinite(x.angle_calibration_rad)) return MI355NDT_ERR_BAD_ARG;     // (NaN, and the infinities whose sine is one)
  memset(c, 0, sizeof *c);
  c->use_df = p.use_distance_filter; c->dnear = p.distance_near; c->dfar = p.distance_far;
  c->leaf = p.downsample_resolution;
  c->downsample = c->leaf > 0.f;
  c->approx = c->downsample && x.downsample_method == MI355NDT_DOWNSAMPLE_APPROX_VOXELGRID;
  c->mv.on = p.use_transform != 0;
  for (int a = 0; a < 3; a++) for (int k = 0; k < 4; k++) c->mv.m[4 * a + k] = p.transform_colmajor[4 * k + a];
  c->cal.on = x.use_angle_calibration != 0;
  c->cal.sn = std::sin(x.angle_calibration_rad); c->cal.cs = std::cos(x.angle_calibration_rad);
  c->ioff = ioff;
  return MI355NDT_OK;
}
// the pitch of a group whose largest raw cloud has maxn points
static size_t pfb_pitch(const PfbChain& c, size_t maxn) {
  return std::max((size_t)64, (maxn + 63) & ~(size_t)63) + (c.approx ? (size_t)PFA_BUCKETS : 0);
}
// The VoxelGrid middle of every chain, for K clouds whose rows X ([cloud][>= 3][rp]), keep flags (w.keep) and extremes (w.mm) are filled and
// whose result words k_pfb_begin has set: grid, keys, the stable sort by voxel index (a cloud one segment), heads, the three scan kernels,
// for both down-sampling methods.  It leaves the emit positions in w.pos, the counts in res[0, K), the overflow word in res[K] and the
// too-small word in res[K + 1] (w.stat), and returns the sorted keys and point ids the emit kernel walks.  Nothing waits.
struct PfbSorted { const unsigned *keys, *vals; };
static PfbSorted pfb_positions(hipStream_t s, VoxelScratch& w, const PfbChain& c, const float* X, const PfbItem* items, int K, size_t rp) {
  const int tiles = (int)((rp + RS_TILE - 1) / RS_TILE);  // of one cloud: sort tiles = scan chunks (RS_TILE == PF_SCAN_CHUNK)
  static_assert(RS_TILE == PF_SCAN_CHUNK, "one tile count serves the sort and the scan");
  int* res = w.stat;
  const size_t seg = (size_t)K * rp;               // (the sort's second key / id arrays start here)
  const unsigned* keys = w.keys; const unsigned* vals = w.vals;
  if (c.approx) {
    k_pfa_grid<<<(K + 63) / 64, 64, 0, s>>>(w.mm, c.leaf, w.grid, items, K, res);
    k_pfa_keys<<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, items, K, tiles, w.keep, w.grid, w.keys, w.flag);
    const RsPlan plan = rs_plan(10);               // 513 key values: one pass
    assert(rs_disjoint(w.keys, w.vals, w.keys + seg, w.vals + seg, seg));
    rs_pass(s, plan.bits, w.keys, w.vals, w.keys + seg, w.vals + seg, rp, 0, w.hist, w.offs, tiles, K, true);
    keys = w.keys + seg; vals = w.vals + seg;
    k_pfa_heads<<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, keys, vals, w.keep, items, K, tiles, w.grid, w.flag);
  } else {
    if (c.downsample) {
      const RsPlan plan = rs_plan(31);
      k_pfb_grid<<<(K + 63) / 64, 64, 0, s>>>(w.mm, c.leaf, w.grid, items, K, res);
      k_pfb_keys<<<xcd_grid(tiles, K), 256, 0, s>>>(X, rp, items, K, tiles, w.keep, w.grid, w.keys);
      unsigned *ka = w.keys, *va = w.vals, *kb = w.keys + seg, *vb = w.vals + seg;
      assert(rs_disjoint(ka, va, kb, vb, seg));
      for (int ps = 0; ps < plan.passes; ps++) {
        rs_pass(s, plan.bits, ka, va, kb, vb, rp, ps * plan.bits, w.hist, w.offs, tiles, K, ps == 0);
        std::swap(ka, kb); std::swap(va, vb);
      }
      keys = ka; vals = va;
    }
    k_pfb_heads<<<xcd_grid(tiles, K), 256, 0, s>>>(keys, w.keep, rp, items, K, tiles, w.grid, c.downsample, w.flag);
  }
  k_pfb_scan_totals<<<xcd_grid(tiles, K), 1024, 0, s>>>(w.flag, rp, w.tmp, tiles, K);
  k_pfb_scan_offsets<<<K, 1024, 0, s>>>(w.tmp, tiles, items, K, res);
  k_pfb_scan_apply<<<xcd_grid(tiles, K), 1024, 0, s>>>(w.flag, rp, w.tmp, w.pos, tiles, K);
  return PfbSorted{keys, vals};
}
// The chain over the K clouds staged in the scratch (rows in w.in at pitch rp, their items in w.tab): every stage one launch, the filtered
// points into the items' rows, the result words (PFB_RES_WORDS) in w.stat.  Nothing waits.  pi.in not null: the group's intensity plane and
// where every cloud's filtered intensities go; the emit kernels' INTENSITY instantiations run.
static void pfb_enqueue(hipStream_t s, VoxelScratch& w, const PfbChain& c, int K, size_t rp, const PfbInt pi) {
  const int tiles = (int)((rp + RS_TILE - 1) / RS_TILE);
  const PfbItem* items = (const PfbItem*)(unsigned char*)w.tab;
  k_pfb_begin<<<(6 * K + 255) / 256, 256, 0, s>>>(w.mm, w.stat, K);
  const int fx = std::max(1, std::min(tiles * (RS_TILE / 256) / 4, 32));   // flag workgroups per cloud: four points per thread and pass, 32 at the most
  k_pfb_flag<<<xcd_grid(fx, K), 256, 0, s>>>(w.in, rp, items, K, fx, c.use_df, c.dnear, c.dfar, c.mv, c.cal, w.keep, w.mm);
  const PfbSorted v = pfb_positions(s, w, c, w.in, items, K, rp);
  if (c.approx) {
    if (pi.in) k_pfa_emit<true><<<xcd_grid(tiles, K), 256, 0, s>>>(w.in, rp, v.keys, v.vals, w.keep, w.flag, w.pos, w.grid, items, K, tiles, pi);
    else k_pfa_emit<false><<<xcd_grid(tiles, K), 256, 0, s>>>(w.in, rp, v.keys, v.vals, w.keep, w.flag, w.pos, w.grid, items, K, tiles, pi);
  } else {
    if (pi.in) k_pfb_emit<true><<<xcd_grid(tiles, K), 256, 0, s>>>(w.in, rp, v.keys, v.vals, w.flag, w.pos, w.grid, c.downsample, items, K, tiles, pi);
    else k_pfb_emit<false><<<xcd_grid(tiles, K), 256, 0, s>>>(w.in, rp, v.keys, v.vals, w.flag, w.pos, w.grid, c.downsample, items, K, tiles, pi);
  }
}
// Staging the intensity of a group of K clouds: the plane lies behind the group's rows in w.in, the K row pointers behind the K items in the
// table block.  With the calibration on nothing is staged: vertical_angle_calibration's fresh points carry intensity 0, so the plane is
// zeroed and every sum, every kept point comes out +0.0f.
static float* pfb_plane(VoxelScratch& w, int K, size_t rp) { return w.in + (size_t)3 * K * rp; }
static float** pfb_plane_out(unsigned char* tab, int K) { return (float**)(tab + (size_t)K * sizeof(PfbItem)); }
static_assert(sizeof(PfbItem) % 8 == 0, "the row pointers behind the items");

// how many clouds of pitch rp a group holds: the caller's own number (pf_group), else what the scratch budget allows at `point_bytes` per
// position; never more than PFB_GROUP_MAX or the call's `clouds`
static int pfb_group_size(const mi355ndt_handle* h, size_t point_bytes, size_t rp, int clouds) {
  const int group = h->pf_group > 0 ? h->pf_group : (int)std::min((size_t)PFB_GROUP_MAX, std::max((size_t)1, PFB_SCRATCH_BUDGET / (point_bytes * rp)));
  return std::min(std::min(group, PFB_GROUP_MAX), clouds);
}

// kernels_ms (may be null): the time of the prefilter's kernels, HIP events around every group's chain, summed
static int batch_prefilter_impl(mi355ndt_handle* h, int first_pair, int n, const void* const* targets, const size_t* target_counts,
                                const void* const* sources, const size_t* source_counts, size_t stride, const mi355ndt_prefilter_params* prm,
                                size_t* target_counts_out, size_t* source_counts_out, double* kernels_ms) {
  // every argument before anything is staged: a refused call changes nothing
  if (n <= 0 || first_pair < 0 || first_pair + n > h->n_pairs || (!targets && !sources) || (targets && !target_counts) || (sources && !source_counts))
    return MI355NDT_ERR_BAD_ARG;
  if (h->d_tgt != h->d_tgt_own || h->d_src != h->d_src_own) return MI355NDT_ERR_BAD_ARG;
  bool any = false;
  for (int k = 0; k < n; k++) any = any || (targets && target_counts[k]) || (sources && source_counts[k]);
  PfbChain chain;
  if (pfb_chain(prm, any ? stride : 0, &chain)) return MI355NDT_ERR_BAD_ARG;
  const bool with_i = chain.ioff >= 0;
  struct Raw { bool tgt; int pair; const void* pts; size_t n; };
  std::vector<Raw> raw;                                 // pair after pair, the target before the source: "the first slot that ..." follows this order
  size_t maxn = 0;
  for (int k = 0; k < n; k++)
    for (int side = 0; side < 2; side++) {
      const void* const* cl = side == 0 ? targets : sources;
      if (!cl) continue;
      const size_t c = (side == 0 ? target_counts : source_counts)[k];
      if (c && (!cl[k] || stride < 12 || c >= (1u << 30))) return MI355NDT_ERR_BAD_ARG;
      raw.push_back(Raw{side == 0, first_pair + k, cl[k], c});
      maxn = std::max(maxn, c);
    }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int n_raw = (int)raw.size();
  const size_t rp = pfb_pitch(chain, maxn);
  const int group = pfb_group_size(h, PFB_POINT_BYTES + (with_i ? 4 : 0), rp, n_raw);
  VoxelScratch& w = h->vs;
  VsNeed need;
  need.clouds = (size_t)group; need.pitch = (size_t)group * rp; need.in = (with_i ? 4 : 3) * need.pitch;
  need.tab = (size_t)group * (sizeof(PfbItem) + (with_i ? sizeof(float*) : 0)); need.stat = PFB_RES_WORDS(group);
  int rc = vs_reserve(h, need);
  if (rc) return rc;
  if (with_i) {                                    // the sides' intensity planes, [slot][pitch] beside the rows (zeroed below, with the rows)
    if (targets) HIPCHK(h, h->d_tgt_i.reserve((size_t)h->n_pairs * h->tgt_pitch));
    if (sources) HIPCHK(h, h->d_src_i.reserve((size_t)h->n_pairs * h->src_pitch));
  }
  // until the counts are known the touched slots hold nothing: an error half way leaves no valid-looking cloud or grid over rows being rewritten
  const std::vector<int> zeros((size_t)n, 0);
  if (targets) cloud_changed(h, true, first_pair, n, zeros.data());
  if (sources) cloud_changed(h, false, first_pair, n, zeros.data());
  HipEvent ev[2];
  if (kernels_ms) { *kernels_ms = 0.0; for (auto& e : ev) HIPCHK(h, e.create(hipEventDefault)); }
  std::vector<int> counts((size_t)n_raw, 0);
  int first_overflow = INT_MAX, first_small = INT_MAX;
  for (int g0 = 0; g0 < n_raw; g0 += group) {
    const int K = std::min(group, n_raw - g0);
    if (w.pending) { HIPCHK(h, hipStreamSynchronize(s)); w.pending = false; }
    PfbItem* tab = (PfbItem*)(unsigned char*)w.h_tab;
    std::vector<UpItem> up((size_t)K);
    for (int k = 0; k < K; k++) {
      const Raw& r = raw[(size_t)(g0 + k)];
      const size_t dp = r.tgt ? h->tgt_pitch : h->src_pitch;
      tab[k] = PfbItem{(r.tgt ? h->d_tgt_own : h->d_src_own) + (size_t)r.pair * 3 * dp, (unsigned long long)dp, (int)r.n, g0 + k};
      up[(size_t)k] = UpItem{w.in, rp, k, r.pts, r.n, stride};
      if (with_i) {
        pfb_plane_out(w.h_tab, K)[k] = (r.tgt ? h->d_tgt_i : h->d_src_i) + (size_t)r.pair * dp;
        if (!chain.cal.on) { up[(size_t)k].ioff = chain.ioff; up[(size_t)k].d_i = pfb_plane(w, K, rp) + (size_t)k * rp; }
      }
    }
    const PfbInt pi = {with_i ? pfb_plane(w, K, rp) : nullptr, with_i ? pfb_plane_out(w.tab, K) : nullptr};
    w.pending = true;
    HIPCHK(h, hipMemcpyAsync(w.tab, w.h_tab, (size_t)K * (sizeof(PfbItem) + (with_i ? sizeof(float*) : 0)), hipMemcpyHostToDevice, s));
    rc = upload_items_grouped(h, up);
    if (rc) return rc;
    rc = uploads_before_compute(h);
    if (rc) return rc;
    if (g0 == 0) {
      // the rows behind a count are zero, as an upload leaves them: the touched slots are one contiguous range per side
      if (targets) HIPCHK(h, hipMemsetAsync(h->d_tgt_own + (size_t)first_pair * 3 * h->tgt_pitch, 0, (size_t)n * 3 * h->tgt_pitch * sizeof(float), s));
      if (sources) HIPCHK(h, hipMemsetAsync(h->d_src_own + (size_t)first_pair * 3 * h->src_pitch, 0, (size_t)n * 3 * h->src_pitch * sizeof(float), s));
      if (with_i && targets) HIPCHK(h, hipMemsetAsync(h->d_tgt_i + (size_t)first_pair * h->tgt_pitch, 0, (size_t)n * h->tgt_pitch * sizeof(float), s));
      if (with_i && sources) HIPCHK(h, hipMemsetAsync(h->d_src_i + (size_t)first_pair * h->src_pitch, 0, (size_t)n * h->src_pitch * sizeof(float), s));
    }
    if (with_i && chain.cal.on) HIPCHK(h, hipMemsetAsync(pi.in, 0, (size_t)K * rp * sizeof(float), s));
    if (kernels_ms) HIPCHK(h, hipEventRecord(ev[0], s));
    int* res = w.stat;
    pfb_enqueue(s, w, chain, K, rp, pi);
    if (kernels_ms) HIPCHK(h, hipEventRecord(ev[1], s));
    rc = compute_enqueued(h);                      // the next group's uploads into the scratch wait for these kernels
    if (rc) return rc;
    // the group's one wait: K counts and the two "first cloud that ..." words
    int* ret = w.h_ret;
    HIPCHK(h, hipMemcpyAsync(ret, res, PFB_RES_WORDS(K) * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    w.pending = false;
    HIPCHK(h, hipGetLastError());
    if (kernels_ms) { float ms = 0.f; HIPCHK(h, hipEventElapsedTime(&ms, ev[0], ev[1])); *kernels_ms += ms; }
    for (int k = 0; k < K; k++) counts[(size_t)(g0 + k)] = ret[k];
    first_overflow = std::min(first_overflow, ret[K]);
    first_small = std::min(first_small, ret[K + 1]);
  }
  if (first_overflow != INT_MAX) {                  // (the touched slots stay recorded as empty)
    const Raw& r = raw[(size_t)first_overflow];
    h->err = "batch prefilter: the filtered " + std::string(r.tgt ? "target" : "source") + " of slot " + std::to_string(r.pair) + " has " +
             std::to_string(counts[(size_t)first_overflow]) + " points, more than its slot holds (" + std::to_string(r.tgt ? h->tgt_pitch : h->src_pitch) +
             "): reserve the batch for the filtered clouds";
    return MI355NDT_ERR_BAD_ARG;
  }
  for (int j = 0; j < n_raw; j++) {
    const Raw& r = raw[(size_t)j];
    cloud_changed(h, r.tgt, r.pair, (size_t)counts[(size_t)j], with_i);
    size_t* out = r.tgt ? target_counts_out : source_counts_out;
    if (out) out[r.pair - first_pair] = (size_t)counts[(size_t)j];
  }
  if (first_small != INT_MAX) {
    const Raw& r = raw[(size_t)first_small];
    const std::string what = std::string(r.tgt ? "target" : "source") + " of slot " + std::to_string(r.pair);
    h->err = "batch prefilter: leaf size too small for the extent of the " + what + ", voxel indices would overflow; " + what + " not down-sampled";
  }
  return MI355NDT_OK;
}

int mi355ndt_batch_prefilter(mi355ndt_handle* h, int first_pair, int n, const void* const* targets, const size_t* target_counts,
                             const void* const* sources, const size_t* source_counts, size_t stride, const mi355ndt_prefilter_params* p,
                             size_t* target_counts_out, size_t* source_counts_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  const int rc = batch_prefilter_impl(h, first_pair, n, targets, target_counts, sources, source_counts, stride, p, target_counts_out, source_counts_out, nullptr);
  // an error exit may leave copies and kernels queued that still use the scratch and the slot rows: later uploads wait for them all the same
  if (rc != MI355NDT_OK && rc != MI355NDT_ERR_BAD_ARG && h->ev_compute) (void)compute_enqueued(h);
  return rc;
}

// One cloud into the resident result: the batch chain over a group of ONE cloud.  (The arguments have been checked.)
static int prefilter_one(mi355ndt_handle* h, const void* pts, size_t n, size_t stride, const PfbChain& chain,
                         void* out_pts, size_t out_capacity, size_t out_stride, size_t* n_out) {
  const bool with_i = chain.ioff >= 0;
  const size_t ch = with_i ? 4 : 3;
  *n_out = 0;
  h->pf_count = 0; h->pf_resident = true;          // (until the count is known the result is an empty one of the shape it had)
  if (n == 0) { h->pf_ch = (int)ch; h->pf_ioff = chain.ioff; h->pf_pitch = 0; return MI355NDT_OK; }   // an empty result: no row of the buffer is its own
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t pitch = (n + 63) & ~(size_t)63, rp = pfb_pitch(chain, n);
  VoxelScratch& w = h->vs;
  VsNeed need;
  need.pitch = rp; need.in = ch * rp; need.tab = sizeof(PfbItem) + sizeof(float*); need.stat = PFB_RES_WORDS(1);
  int rc = vs_reserve(h, need);
  if (rc) return rc;
  if (ch * pitch > h->d_pf_out.cap) HIPCHK(h, hipStreamSynchronize(s));   // (the result buffer is re-allocated: no copy out of it may still run)
  HIPCHK(h, h->d_pf_out.reserve(ch * pitch));
  h->pf_pitch = pitch; h->pf_ch = (int)ch; h->pf_ioff = chain.ioff;   // (the buffer holds [ch][pitch] from here on)
  PfbItem* tab = (PfbItem*)(unsigned char*)w.h_tab;
  tab[0] = PfbItem{h->d_pf_out, (unsigned long long)pitch, (int)n, 0};
  pfb_plane_out(w.h_tab, 1)[0] = h->d_pf_out + 3 * pitch;              // (the result's fourth row, when it has one)
  const PfbInt pi = {with_i ? pfb_plane(w, 1, rp) : nullptr, with_i ? pfb_plane_out(w.tab, 1) : nullptr};
  w.pending = true;
  HIPCHK(h, hipMemcpyAsync(w.tab, w.h_tab, sizeof(PfbItem) + sizeof(float*), hipMemcpyHostToDevice, s));
  UpItem up = {w.in, rp, 0, pts, n, stride};
  if (with_i && !chain.cal.on) { up.ioff = chain.ioff; up.d_i = pi.in; }
  rc = upload_items(h, &up, 1);
  if (rc) return rc;
  rc = uploads_before_compute(h);
  if (rc) return rc;
  if (with_i && chain.cal.on) HIPCHK(h, hipMemsetAsync(pi.in, 0, rp * sizeof(float), s));
  pfb_enqueue(s, w, chain, 1, rp, pi);
  int* ret = w.h_ret;
  HIPCHK(h, hipMemcpyAsync(ret, w.stat, PFB_RES_WORDS(1) * sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  w.pending = false;
  HIPCHK(h, hipGetLastError());
  const size_t m = (size_t)ret[0];                // (at most n: the result's pitch holds it)
  h->pf_count = (int)m;
  *n_out = m;
  if (ret[2] != INT_MAX) h->err = "prefilter: leaf size too small for the cloud's extent, voxel indices would overflow; cloud not down-sampled";
  return pf_result_records(h, m, out_pts, out_capacity, out_stride);
}

// replaces PrefilteringNodelet::distance_filter + downsample (prefiltering_nodelet.cpp:137-181): mi355ndt_prefilter_p with plain parameters --
// no move, no calibration, VOXELGRID
int mi355ndt_prefilter(mi355ndt_handle* h, const void* pts, size_t n, size_t stride,
                       int use_distance_filter, double distance_near, double distance_far, float downsample_resolution,
                       void* out_pts, size_t out_capacity, size_t out_stride, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if ((!pts && n) || (n && stride < 12) || n >= (1u << 30) || !n_out || (out_pts && out_stride < 12)) return MI355NDT_ERR_BAD_ARG;
  mi355ndt_prefilter_params p;
  (void)mi355ndt_prefilter_params_default(&p);
  p.use_distance_filter = use_distance_filter; p.distance_near = distance_near; p.distance_far = distance_far;
  p.downsample_resolution = downsample_resolution;
  PfbChain chain;
  if (pfb_chain(&p, 0, &chain)) return MI355NDT_ERR_BAD_ARG;     // (a NaN resolution)
  return prefilter_one(h, pts, n, stride, chain, out_pts, out_capacity, out_stride, n_out);
}

// mi355ndt_prefilter with the nodelet's whole parameter set
int mi355ndt_prefilter_p(mi355ndt_handle* h, const void* pts, size_t n, size_t stride, const mi355ndt_prefilter_params* prm,
                         void* out_pts, size_t out_capacity, size_t out_stride, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if ((!pts && n) || (n && stride < 12) || n >= (1u << 30) || !n_out || (out_pts && out_stride < 12)) return MI355NDT_ERR_BAD_ARG;
  PfbChain chain;
  if (pfb_chain(prm, n ? stride : 0, &chain)) return MI355NDT_ERR_BAD_ARG;
  if (chain.ioff >= 0 && out_pts && (size_t)chain.ioff + 4 > out_stride) {   // (the result's intensity goes out at the input's offset)
    h->err = "prefilter_p: the intensity goes out at byte " + std::to_string(chain.ioff) + " of a record; out_stride_bytes " + std::to_string(out_stride) +
             " cannot hold it";
    return MI355NDT_ERR_BAD_ARG;
  }
  return prefilter_one(h, pts, n, stride, chain, out_pts, out_capacity, out_stride, n_out);
}

// the points a batch slot holds, whatever route filled it; ioff >= 0: with the slot's intensity at that offset of every record (zeros for a
// slot that carries none)
static int batch_get_cloud_impl(mi355ndt_handle* h, int pair, int role, void* out_pts, size_t out_capacity, size_t out_stride, int ioff, size_t* n_out) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (pair < 0 || pair >= h->n_pairs || (role != 1 && role != 2) || !n_out || (out_pts && out_stride < 12)) return MI355NDT_ERR_BAD_ARG;
  if (out_pts && ioff >= 0 && (ioff < 12 || ioff % 4 != 0 || (size_t)ioff + 4 > out_stride)) return MI355NDT_ERR_BAD_ARG;
  const bool tgt = role == 2;
  const float* base = tgt ? h->d_tgt : h->d_src;
  const size_t pitch = tgt ? h->tgt_pitch : h->src_pitch;
  const size_t m = (size_t)(tgt ? h->h_tgt_cnt : h->h_src_cnt)[(size_t)pair];
  *n_out = m;
  if (!out_pts || m == 0) return MI355NDT_OK;
  if (m > out_capacity || !base) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));   // pending uploads and kernels
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const float* irow = ioff >= 0 ? slot_intensity_row(h, tgt, pair) : nullptr;
  std::vector<float> tmp((irow ? 4 : 3) * m);
  for (int a = 0; a < 3; a++)
    HIPCHK(h, hipMemcpy(tmp.data() + (size_t)a * m, base + (size_t)pair * 3 * pitch + (size_t)a * pitch, m * sizeof(float), hipMemcpyDeviceToHost));
  if (irow) HIPCHK(h, hipMemcpy(tmp.data() + 3 * m, irow, m * sizeof(float), hipMemcpyDeviceToHost));
  rows_to_records(tmp.data(), m, irow ? 4 : 3, m, out_pts, out_stride, ioff);
  return MI355NDT_OK;
}
int mi355ndt_batch_get_cloud(mi355ndt_handle* h, int pair, int role, void* out_pts, size_t out_capacity, size_t out_stride, size_t* n_out) {
  return batch_get_cloud_impl(h, pair, role, out_pts, out_capacity, out_stride, -1, n_out);
}
int mi355ndt_batch_get_cloud_i(mi355ndt_handle* h, int pair, int role, void* out_pts, size_t out_capacity, size_t out_stride_bytes,
                               int out_intensity_offset_bytes, size_t* n_out) {
  if (out_intensity_offset_bytes < 0) return !h ? MI355NDT_ERR_BAD_HANDLE : MI355NDT_ERR_BAD_ARG;
  return batch_get_cloud_impl(h, pair, role, out_pts, out_capacity, out_stride_bytes, out_intensity_offset_bytes, n_out);
}
