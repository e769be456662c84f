// ndt_host_upload.hpp -- capacity management (reserve, bind) and the host-cloud uploads: pinned staging ring, copy streams, upload_items and its
// staging threads, mi355ndt_batch_set_* / mi355ndt_batch_set_clouds, the two events that order uploads against compute, and the device-to-device
// copy of rows into a batch slot.
#pragma once

// ---- capacity management ----------------------------------------------------------------------
static int ensure_pair_arrays(mi355ndt_handle* h, int n_pairs) {
  if (n_pairs <= h->cap_pairs) return MI355NDT_OK;
  for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the arrays are released and re-created one by one: until all of them exist again the engine holds no batch at all
  // (a failure half way must not leave cap_pairs vouching for freed or undersized buffers)
  h->cap_pairs = 0; h->n_pairs = 0; h->d_tgt_cnt = h->d_src_cnt = nullptr; h->d_guess = nullptr;
  clouds_reset(h, true, true); h->aligned_once = false;
  HIPCHK(h, h->d_tgt_cnt_own.realloc_exact(n_pairs)); h->d_tgt_cnt = h->d_tgt_cnt_own;
  HIPCHK(h, h->d_src_cnt_own.realloc_exact(n_pairs)); h->d_src_cnt = h->d_src_cnt_own;
  h->up_tgt_cnt.clear(); h->up_src_cnt.clear();       // fresh device arrays: nothing uploaded yet
  HIPCHK(h, h->d_grid.realloc_exact(n_pairs));
  HIPCHK(h, h->d_nwords.realloc_exact(n_pairs + 2));
  // build control words, zeroed by ONE memset per build: [0] total bitmap words, [1] largest grid, then per target six extremes
  // (k_minmax's encoding makes zero "none yet")
  HIPCHK(h, h->d_word_off.realloc_exact(2 + 6 * (size_t)n_pairs));
  h->d_minmax = h->d_word_off + 2;
  HIPCHK(h, h->d_state.realloc_exact(n_pairs));
  HIPCHK(h, h->d_guess_own.realloc_exact((size_t)n_pairs * 16)); h->d_guess = h->d_guess_own;
  HIPCHK(h, h->h_pin_guess.realloc_exact((size_t)n_pairs * 16));
  HIPCHK(h, h->d_results.realloc_exact(n_pairs));
  HIPCHK(h, h->d_active_list.realloc_exact(n_pairs));
  HIPCHK(h, hipMemsetAsync(h->d_grid, 0, n_pairs * sizeof(GridDesc), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_state, 0, n_pairs * sizeof(PairState), h->stream));
  h->cap_pairs = n_pairs;
  h->h_tgt_cnt.assign(n_pairs, 0);
  h->h_src_cnt.assign(n_pairs, 0);
  return MI355NDT_OK;
}

static int alloc_side(mi355ndt_handle* h, bool tgt, int n_pairs, size_t pitch) {
  DevBuf<float>& buf = tgt ? h->d_tgt_own : h->d_src_own;
  size_t& own_pitch = tgt ? h->own_tgt_pitch : h->own_src_pitch;
  int& own_pairs = tgt ? h->own_tgt_pairs : h->own_src_pairs;
  if (buf && own_pitch == pitch && own_pairs == n_pairs) return MI355NDT_OK;
  for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, buf.realloc_exact((size_t)n_pairs * 3 * pitch));
  own_pitch = pitch; own_pairs = n_pairs;
  clouds_reset(h, tgt, !tgt);
  return MI355NDT_OK;
}

int mi355ndt_batch_reserve(mi355ndt_handle* h, int n_pairs, size_t max_tgt, size_t max_src) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (n_pairs <= 0 || max_tgt == 0 || max_src == 0 || n_pairs > MAX_PAIRS) return MI355NDT_ERR_BAD_ARG;
  if (max_tgt >= (1u << 31) || max_src >= (1u << 31)) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  // pitches padded to 64 floats so every row starts 256-B aligned
  size_t tp = (max_tgt + 63) & ~(size_t)63, sp = (max_src + 63) & ~(size_t)63;
  int rc = ensure_pair_arrays(h, n_pairs);
  if (rc) return rc;
  if (n_pairs != h->n_pairs || h->d_tgt != h->d_tgt_own || h->d_src != h->d_src_own) {
    clouds_reset(h, true, true); h->aligned_once = false;
  }
  rc = alloc_side(h, true, n_pairs, tp);
  if (rc == MI355NDT_OK) rc = alloc_side(h, false, n_pairs, sp);
  if (rc) return rc;
  if (h->d_tgt_i || h->d_src_i) {                 // the slots' intensity planes go: the next batch prefilter with an intensity makes them anew
    for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamSynchronize(cs));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->d_tgt_i = DevBuf<float>(); h->d_src_i = DevBuf<float>();
  }
  h->tgt_has_i.assign((size_t)n_pairs, 0); h->src_has_i.assign((size_t)n_pairs, 0);
  h->n_pairs = n_pairs;
  h->tgt_pitch = tp; h->src_pitch = sp;
  h->d_tgt = h->d_tgt_own; h->d_src = h->d_src_own;
  return MI355NDT_OK;
}

// The compute stream must not start before the uploads enqueued so far have landed, and an upload must not overwrite rows a
// kernel enqueued earlier still reads: the two streams hand over through two events.
static int uploads_before_compute(mi355ndt_handle* h) {
  std::lock_guard<std::mutex> lk(h->up_mtx);
  if (h->uploads_pending) {
    for (int i = 0; i < mi355ndt_handle::UP_STREAMS; i++) {
      HIPCHK(h, hipEventRecord(h->ev_uploads[i], h->copy_stream[i]));
      HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_uploads[i], 0));
    }
    h->uploads_pending = false;
  }
  return MI355NDT_OK;
}
static int compute_enqueued(mi355ndt_handle* h) {       // call after enqueueing kernels that read the cloud buffers
  std::lock_guard<std::mutex> lk(h->up_mtx);
  HIPCHK(h, hipEventRecord(h->ev_compute, h->stream));
  for (hipStream_t cs : h->copy_stream) HIPCHK(h, hipStreamWaitEvent(cs, h->ev_compute, 0));
  return MI355NDT_OK;
}

// Host clouds -> SoA rows of their pair slots, asynchronously, SEVERAL CLOUDS PER TRANSFER.  Returns as soon as the caller's memory is no longer
// needed (the records are compacted into a pinned ring slot; nothing of the caller's buffers is referenced afterwards).  One transfer = one
// hipMemcpyAsync + one k_deinterleave_multi launch + one event, whatever the number of clouds in it: with one cloud per transfer the ~50 us of
// HIP calls per cloud, serialised under the engine's lock, held the staging of a 271-pair batch to 60 GB/s of records read whatever the number
// of staging threads (round 6, tools/host_stage_probe.cpp: the same compaction alone reaches 180-195 GB/s at eight threads on the same host).
// ioff >= 0: the record's f32 at that byte offset (its intensity) travels as a fourth word and lands in a fourth row: behind x, y, z, or --
// d_i not null -- in the `pitch` floats at d_i
struct UpItem { float* d_base; size_t pitch; int pair; const void* pts; size_t n, stride; int ioff = -1; float* d_i = nullptr; };
static int upload_items(mi355ndt_handle* h, const UpItem* it, int cnt) {
  if (cnt < 1 || cnt > UP_GROUP_MAX) return MI355NDT_ERR_BAD_ARG;
  size_t total = 0;                               // words staged: 3 per point (4 with the intensity, each such cloud starting on a 16-byte boundary)
  for (int k = 0; k < cnt; k++) {
    if (!it[k].pts && it[k].n) return MI355NDT_ERR_BAD_ARG;
    if ((it[k].n && it[k].stride < 12) || it[k].n > it[k].pitch) return MI355NDT_ERR_BAD_ARG;
    if (it[k].n && it[k].ioff >= 0 && (size_t)it[k].ioff + 4 > it[k].stride) return MI355NDT_ERR_BAD_ARG;
    if (it[k].ioff >= 0) total = (total + 3) & ~(size_t)3;
    total += (it[k].ioff >= 0 ? 4 : 3) * it[k].n;
  }
  mi355ndt_handle::UpSlot* u = nullptr;
  for (;;) {                                      // a slot no other thread is filling right now
    {
      std::lock_guard<std::mutex> lk(h->up_mtx);
      for (int t = 0; t < mi355ndt_handle::UP_SLOTS && !u; t++) {
        mi355ndt_handle::UpSlot* c = &h->up[(h->up_next + t) % mi355ndt_handle::UP_SLOTS];
        if (!c->filling) { u = c; h->up_next = (h->up_next + t + 1) % mi355ndt_handle::UP_SLOTS; c->filling = true; }
      }
    }
    if (u) break;
    std::this_thread::yield();                    // more uploader threads than slots
  }
  hipError_t e = hipSuccess;
  if (!u->ev) e = u->ev.create();
  if (e == hipSuccess && u->used) e = hipEventSynchronize(u->ev);      // the slot's previous transfer has to be out of the pinned buffer
  if (e == hipSuccess && total > std::min(u->h.cap, u->d.cap)) {
    u->used = false;
    const size_t cap = std::max(total, (size_t)3 * 65536);
    e = u->h.realloc_exact(cap);
    if (e == hipSuccess) e = u->d.realloc_exact(cap);
  }
  if (e != hipSuccess) {
    std::lock_guard<std::mutex> lk(h->up_mtx);
    h->err = std::string("upload staging: ") + hipGetErrorString(e);
    u->filling = false;
    return MI355NDT_ERR_HIP;
  }
  // the CPU part, outside the lock: x,y,z (and the intensity, where asked for) of every record into the pinned slot, cloud after cloud
  DeintTab tab;
  tab.cnt = cnt;
  size_t off = 0, max_pitch = 0;                  // off: words
  for (int k = 0; k < cnt; k++) {
    const unsigned char* p = (const unsigned char*)it[k].pts;
    const size_t n = it[k].n, stride = it[k].stride;
    const int ioff = it[k].ioff;
    if (ioff >= 0) off = (off + 3) & ~(size_t)3;
    float* dst = u->h + off;
    if (ioff >= 0) {
      if (stride == 16 && ioff == 12) { if (n) memcpy(dst, p, n * 16); }
      else for (size_t i = 0; i < n; i++) { memcpy(dst + 4 * i, p + i * stride, 12); memcpy(dst + 4 * i + 3, p + i * stride + ioff, 4); }
    } else if (stride == 12) { if (n) memcpy(dst, p, n * 12); }
    else for (size_t i = 0; i < n; i++) memcpy(dst + 3 * i, p + i * stride, 12);
    tab.e[k].src_off = off; tab.e[k].n = (int)n; tab.e[k].w4 = ioff >= 0; tab.e[k].rows = it[k].d_base + (size_t)it[k].pair * 3 * it[k].pitch; tab.e[k].pitch = it[k].pitch;
    tab.e[k].row4 = it[k].d_i ? it[k].d_i : tab.e[k].rows + 3 * it[k].pitch;
    off += (ioff >= 0 ? 4 : 3) * n;
    max_pitch = std::max(max_pitch, it[k].pitch);
  }
  {
    std::lock_guard<std::mutex> lk(h->up_mtx);
    // the copy stream is chosen by DESTINATION (the pair slot's group), not by staging slot: two uploads into the same rows -- set_source(A)
    // then set_source(B) with no build / align in between -- ride one stream and land in call order (a group never spans two stream classes:
    // mi355ndt_batch_set_clouds groups pairs by pair / UP_GROUP_PAIRS)
    hipStream_t cs = h->copy_stream[(it[0].pair / UP_GROUP_PAIRS) % mi355ndt_handle::UP_STREAMS];
    if (total) e = hipMemcpyAsync(u->d, u->h, total * sizeof(float), hipMemcpyHostToDevice, cs);
    if (e == hipSuccess) {
      k_deinterleave_multi<<<dim3((unsigned)((max_pitch + 255) / 256), (unsigned)cnt), 256, 0, cs>>>(u->d, tab);
      e = hipEventRecord(u->ev, cs);
    }
    u->used = e == hipSuccess;
    u->filling = false;
    h->uploads_pending = true;
    h->P.cloud_uploads += cnt;                     // (counted whether or not event profiling is on: tests/test_adaptor.py holds the drop-in to one per frame)
    h->P.cloud_upload_bytes += (long long)(total * sizeof(float));
    h->P.cloud_transfers++;
    if (e != hipSuccess) { h->err = std::string("upload: ") + hipGetErrorString(e); return MI355NDT_ERR_HIP; }
  }
  return MI355NDT_OK;
}
static int upload_cloud(mi355ndt_handle* h, float* d_base, size_t pitch, int pair, const void* pts, size_t n, size_t stride) {
  const UpItem it = {d_base, pitch, pair, pts, n, stride};
  return upload_items(h, &it, 1);
}

// nt staging threads, the caller's among them (t = 0), each running work(t) -> status; the first status that is not OK is returned.  Nothing
// may be thrown across the C boundary: a thread that cannot be created (std::system_error) just means the others -- at least the caller's --
// do its share.
template <typename Work>
static int staging_threads(int nt, Work work) {
  std::vector<int> rcs((size_t)nt, MI355NDT_OK);
  std::vector<std::thread> th;
  try {
    th.reserve((size_t)nt);
    for (int t = 1; t < nt; t++) th.emplace_back([&rcs, &work, t] { rcs[(size_t)t] = work(t); });
  } catch (...) {}
  rcs[0] = work(0);
  for (auto& x : th) x.join();
  for (int rc : rcs) if (rc != MI355NDT_OK) return rc;
  return MI355NDT_OK;
}

// many clouds into rows of one buffer (the map cloud's keyframes, the window's scans): groups of up to UP_GROUP_MAX items, one transfer
// each, staged by up to eight threads
static int upload_items_grouped(mi355ndt_handle* h, const std::vector<UpItem>& items) {
  const int n_groups = (int)((items.size() + UP_GROUP_MAX - 1) / UP_GROUP_MAX);
  std::atomic<int> next_group{0};
  return staging_threads(std::max(1, std::min(8, n_groups)), [&](int) {
    (void)hipSetDevice(h->device);
    for (int g = next_group.fetch_add(1); g < n_groups; g = next_group.fetch_add(1)) {
      const size_t i0 = (size_t)g * UP_GROUP_MAX, i1 = std::min(items.size(), i0 + UP_GROUP_MAX);
      const int rc = upload_items(h, items.data() + i0, (int)(i1 - i0));
      if (rc != MI355NDT_OK) return rc;
    }
    return (int)MI355NDT_OK;
  });
}

// m points of device SoA rows (pitch src_pitch) into a pair slot of the engine's own batch rows, device to device, the slot's rows
// zero-filled up to their pitch as an upload leaves them, and recorded (cloud_changed).  The caller follows with compute_enqueued or a build.
static int rows_into_slot(mi355ndt_handle* h, bool tgt, int pair, const float* rows, size_t src_pitch, size_t m) {
  int rc = uploads_before_compute(h);             // an earlier upload into these rows must not land after the copies (and one into `rows` has to have landed)
  if (rc) return rc;
  const size_t dp = tgt ? h->tgt_pitch : h->src_pitch;
  float* dst = (tgt ? h->d_tgt_own : h->d_src_own) + (size_t)pair * 3 * dp;
  HIPCHK(h, hipMemsetAsync(dst, 0, 3 * dp * sizeof(float), h->stream));
  for (int a = 0; a < 3; a++)
    if (m) HIPCHK(h, hipMemcpyAsync(dst + a * dp, rows + a * src_pitch, m * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  cloud_changed(h, tgt, pair, m);
  return MI355NDT_OK;
}

// one host cloud into its pair slot, target or source side (may be called from several threads, distinct pairs)
static int batch_set_side(mi355ndt_handle* h, bool tgt, int pair, const void* pts, size_t n, size_t stride) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (pair < 0 || pair >= h->n_pairs || (tgt ? h->d_tgt != h->d_tgt_own : h->d_src != h->d_src_own)) return MI355NDT_ERR_BAD_ARG;
  if (hipError_t e = hipSetDevice(h->device)) { std::lock_guard<std::mutex> lk(h->up_mtx); h->err = std::string("hipSetDevice: ") + hipGetErrorString(e); return MI355NDT_ERR_HIP; }
  int rc = upload_cloud(h, tgt ? h->d_tgt_own : h->d_src_own, tgt ? h->tgt_pitch : h->src_pitch, pair, pts, n, stride);
  if (rc == MI355NDT_OK) cloud_changed(h, tgt, pair, n);
  return rc;
}
int mi355ndt_batch_set_target(mi355ndt_handle* h, int pair, const void* pts, size_t n, size_t stride) { return batch_set_side(h, true, pair, pts, n, stride); }
int mi355ndt_batch_set_source(mi355ndt_handle* h, int pair, const void* pts, size_t n, size_t stride) { return batch_set_side(h, false, pair, pts, n, stride); }

// A whole batch of host clouds at once: the engine's own staging threads split the pairs among themselves (staging -- copying x,y,z
// out of the caller's records into pinned memory -- is the CPU-bound part of a host-cloud batch; one thread does ~10 k clouds/s).
int mi355ndt_batch_set_clouds(mi355ndt_handle* h, int first_pair, int n, const void* const* targets, const size_t* target_counts,
                              const void* const* sources, const size_t* source_counts, size_t stride, int n_threads) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  if (n <= 0 || first_pair < 0 || first_pair + n > h->n_pairs || (!targets && !sources) || (targets && !target_counts) || (sources && !source_counts))
    return MI355NDT_ERR_BAD_ARG;
  if (h->d_tgt != h->d_tgt_own || h->d_src != h->d_src_own) return MI355NDT_ERR_BAD_ARG;
  // every pair's arguments before any staging thread starts (what upload_items checks per group): a refused call changes nothing
  for (int k = 0; k < n; k++) {
    const size_t tn = targets ? target_counts[k] : 0, sn = sources ? source_counts[k] : 0;
    if ((tn && (!targets[k] || tn > h->tgt_pitch)) || (sn && (!sources[k] || sn > h->src_pitch)) || ((tn || sn) && stride < 12)) return MI355NDT_ERR_BAD_ARG;
  }
  HIPCHK(h, hipSetDevice(h->device));
  // recorded BEFORE the uploads begin: a HIP failure half way then leaves no valid-looking grids over rows that already hold new points
  if (targets) cloud_changed(h, true, first_pair, n, target_counts);
  if (sources) cloud_changed(h, false, first_pair, n, source_counts);
  const int nt = std::max(1, std::min(n_threads > 0 ? n_threads : 8, n));
  // the engine's own threads stage next to the GPU -- but only on CPUs the CALLER may use: the NUMA node's CPUs intersected with the
  // calling thread's affinity mask (a taskset / cgroup-restricted process keeps its restriction); an empty intersection = no pinning
  cpu_set_t near, mine;
  bool pin = numa_cpus(mi355ndt_host_numa_node(h->device), &near);
  if (pin && sched_getaffinity(0, sizeof mine, &mine) == 0) {
    CPU_AND(&near, &near, &mine);
    pin = CPU_COUNT(&near) > 0;
  } else pin = false;
  // pairs are taken in GROUPS of UP_GROUP_PAIRS consecutive pair slots (aligned to the slot index, so that a slot's uploads always ride the same
  // copy stream): one transfer per group -- both clouds of up to four pairs -- instead of one per cloud (upload_items); a thread that runs slowly
  // (the caller's, t = 0, may sit on a narrowed CPU set) simply takes fewer groups
  const int g_first = first_pair / UP_GROUP_PAIRS, g_last = (first_pair + n - 1) / UP_GROUP_PAIRS;
  std::atomic<int> next_group{g_first};
  auto work = [&](int t) -> int {
    (void)hipSetDevice(h->device);
    if (pin && t > 0) (void)sched_setaffinity(0, sizeof near, &near);   // (t = 0 is the caller's thread: left alone)
    for (int g = next_group.fetch_add(1); g <= g_last; g = next_group.fetch_add(1)) {
      UpItem it[UP_GROUP_MAX];
      int cnt = 0;
      for (int pr = std::max(first_pair, g * UP_GROUP_PAIRS); pr < std::min(first_pair + n, (g + 1) * UP_GROUP_PAIRS); pr++) {
        const int k = pr - first_pair;
        if (targets) it[cnt++] = UpItem{h->d_tgt_own, h->tgt_pitch, pr, targets[k], target_counts[k], stride};
        if (sources) it[cnt++] = UpItem{h->d_src_own, h->src_pitch, pr, sources[k], source_counts[k], stride};
      }
      const int rc = upload_items(h, it, cnt);
      if (rc != MI355NDT_OK) return rc;
    }
    return (int)MI355NDT_OK;
  };
  return staging_threads(nt, work);
}

int mi355ndt_batch_bind_device(mi355ndt_handle* h, int n_pairs, const float* d_t, const int* tc, size_t tp,
                               const float* d_s, const int* scnt, size_t sp) {
  if (!h) return MI355NDT_ERR_BAD_HANDLE;
  NOT_IN_STREAM(h);
  if (n_pairs <= 0 || !d_t || !d_s || !tc || !scnt || tp == 0 || sp == 0 || n_pairs > MAX_PAIRS) return MI355NDT_ERR_BAD_ARG;
  if (tp >= (1u << 31) || sp >= (1u << 31)) return MI355NDT_ERR_BAD_ARG;
  for (int b = 0; b < n_pairs; b++) if (tc[b] < 0 || (size_t)tc[b] > tp || scnt[b] < 0 || (size_t)scnt[b] > sp) return MI355NDT_ERR_BAD_ARG;
  HIPCHK(h, hipSetDevice(h->device));
  int rc = ensure_pair_arrays(h, n_pairs);
  if (rc) return rc;
  h->n_pairs = n_pairs;
  h->d_tgt = d_t; h->d_src = d_s;
  h->tgt_pitch = tp; h->src_pitch = sp;
  cloud_changed(h, true, 0, n_pairs, tc); cloud_changed(h, false, 0, n_pairs, scnt);
  h->aligned_once = false;
  return MI355NDT_OK;
}
