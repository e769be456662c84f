// TEST HELPER (tests/test_segsort_gpu.py): the stable segmented radix sort (ndt_segsort.hpp: k_rs_hist, k_rs_scan, k_rs_scatter behind rs_plan,
// rs_pass, rs_sort_one_segment) and the exclusive scans that turn head flags into emit positions (ndt_prefilter.hpp: k_pf_scan_totals / _offsets /
// _apply; ndt_prefilter_batch.hpp: k_pfb_scan_*, k_pfb_heads) on the device, alone.  It launches the library's own kernels through
// the library's own host entry points and restates none of them; every comparison happens in the test, against numpy.
//
//   segsort_check plan                      no HIP call: prints "f bits passes" of rs_plan(f) for f = 0 .. 33
//   segsort_check run <in.u32> <out.u32>    runs every case of the file
//
// <in.u32>, 32-bit little-endian words: [0x31435353] [mode] [number of cases], then the cases one after the other.
//   mode 1, sort:    [K] [pitch] [field_bits] keys[K * pitch] vals[K * pitch]
//     Two whole sorts, the first with `first` (position i carries id i, vals unused), the second with vals.  K > 1, and K == 1 with `first`,
//     run the rs_pass loop of the batch prefilter; K == 1 without `first` runs rs_sort_one_segment (which takes `first` only with points).
//     Before the first sort one pass at shift 0 runs alone into buffers of its own: its hist and offs are returned.
//     out, per sort: kA vA kB vB hist offs [first only: probe-keys-out probe-vals-out HIST1 OFFS1]; the pair that holds the result is FULL.
//   mode 2, points:  [K] [pitch] [cb] n[K] K x {min_b[3] mul1 mul2 inv_leaf(f32 bits) status} points[K][3][pitch] (f32 bits)
//     The first pass computes the keys (k_rs_hist<BITS, true>); K == 1 runs rs_sort_one_segment with points, K > 1 the rs_pass loop.
//     out: PROBEKEYS probe-vals-in probe-keys-out probe-vals-out HIST1 OFFS1, then kA vA kB vB hist offs as above.
//   mode 3, scans:   [kind] ...
//     kind 0: [n] flags[n]: the chain of exscan_ints.                                  out: TOTALS POS
//     kind 1: [nchunks] totals[nchunks]: k_pf_scan_offsets alone.                      out: TOTALS
//     kind 2: [K] [chunks] [rp] K x {out_pitch n id} flags[K * rp]: the per-cloud chain after k_pfb_begin.   out: mm RES TOTALS POS
//   mode 4, heads:   [K] [rp] [downsample] K x {n status} keys[K * rp] keep[K * rp] (one word per byte)
//     k_pfb_heads over all clouds with every grid's status 0, then with the statuses given.   out: FLAGS_OK FLAGS_PFB
// <out.u32>: the output buffers of every case in the order above, each as [n] [64 guard words] [n words] [64 guard words]; a buffer in capitals
// is written whole, the others with n = 0 (their guard words only).  Every buffer is filled with 0xA5A5A5A5, guards included, before any
// launch: a word the kernels did not write, or wrote outside their buffer, shows in the test.
//   build: as the library (see __graft_entry__.build_segsort_check)
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "ndt_types.hpp"
#include "ndt_segsort.hpp"
#include "ndt_prefilter.hpp"
#include "ndt_prefilter_batch.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(3); } } while (0)
#define REQ(c) do { if (!(c)) { fprintf(stderr, "bad case file: %s (line %d)\n", #c, __LINE__); exit(2); } } while (0)
#define GUARD 64

// a device buffer of n words between two rows of guard words
struct Buf {
  unsigned* base = nullptr;
  size_t n = 0;
  explicit Buf(size_t words) : n(words) {
    CK(hipMalloc((void**)&base, (n + 2 * GUARD) * sizeof(unsigned)));
    CK(hipMemset(base, 0xA5, (n + 2 * GUARD) * sizeof(unsigned)));
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { (void)hipFree(base); }
  unsigned* p() const { return base + GUARD; }
  void put(const unsigned* src, size_t words) const { if (words) CK(hipMemcpy(p(), src, words * sizeof(unsigned), hipMemcpyHostToDevice)); }
  void dump(FILE* f, bool full) const {
    std::vector<unsigned> h(n + 2 * GUARD);
    CK(hipMemcpy(h.data(), base, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    const unsigned hdr = full ? (unsigned)n : 0u;
    bool ok = fwrite(&hdr, 4, 1, f) == 1;
    if (full) ok = ok && fwrite(h.data(), 4, h.size(), f) == h.size();
    else ok = ok && fwrite(h.data(), 4, GUARD, f) == GUARD && fwrite(h.data() + GUARD + n, 4, GUARD, f) == GUARD;
    if (!ok) { perror("write"); exit(2); }
  }
};

struct Reader {
  const unsigned* w; size_t n, at = 0;
  unsigned one() { REQ(at < n); return w[at++]; }
  const unsigned* many(size_t k) { REQ(k <= n - at); const unsigned* r = w + at; at += k; return r; }
};

static void settle() { CK(hipGetLastError()); CK(hipDeviceSynchronize()); }

// the scratch of one sort and what it leaves
struct SortBufs {
  Buf ka, va, kb, vb, hist, offs;
  SortBufs(size_t words, size_t hw) : ka(words), va(words), kb(words), vb(words), hist(hw), offs(hw) {}
  void dump(FILE* f, const unsigned* result_keys) const {
    const bool in_a = result_keys == ka.p();
    ka.dump(f, in_a); va.dump(f, in_a); kb.dump(f, !in_a); vb.dump(f, !in_a); hist.dump(f, false); offs.dump(f, false);
  }
};

// the whole sort: one segment through rs_sort_one_segment where it can express the case, else the pass loop of the batch prefilter
static const unsigned* sort_all(const SortBufs& b, int K, size_t pitch, int field_bits, bool first, const RsPoints* points) {
  const int tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
  if (K == 1 && first == (points != nullptr)) {
    const RsSorted r = rs_sort_one_segment(0, field_bits, b.ka.p(), b.va.p(), b.kb.p(), b.vb.p(), pitch, b.hist.p(), b.offs.p(), points);
    settle();
    return r.keys;
  }
  const RsPlan plan = rs_plan(field_bits);
  unsigned *ka = b.ka.p(), *va = b.va.p(), *kb = b.kb.p(), *vb = b.vb.p();
  for (int ps = 0; ps < plan.passes; ps++) {
    rs_pass(0, plan.bits, ka, va, kb, vb, pitch, ps * plan.bits, b.hist.p(), b.offs.p(), tiles, K, first && ps == 0, ps == 0 ? points : nullptr);
    std::swap(ka, kb); std::swap(va, vb);
  }
  settle();
  return ka;
}

static size_t hist_words(int K, size_t pitch, int field_bits) {
  return (size_t)K * ((pitch + RS_TILE - 1) / RS_TILE) * ((size_t)1 << rs_plan(field_bits).bits);
}

static void case_sort(Reader& in, FILE* out) {
  const int K = (int)in.one();
  const size_t pitch = in.one();
  const int fb = (int)in.one();
  REQ(K >= 1 && K <= 64 && pitch >= 1 && pitch <= (1u << 22) && fb >= 1 && fb <= 32);
  const size_t words = (size_t)K * pitch, hw = hist_words(K, pitch, fb);
  const unsigned* keys = in.many(words);
  const unsigned* vals = in.many(words);
  const int tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
  for (int first = 1; first >= 0; first--) {
    SortBufs b(words, hw);
    b.ka.put(keys, words);
    if (!first) b.va.put(vals, words);
    if (first) {                                                               // the first pass alone: its histogram and offsets
      Buf k2(words), v2(words), hist1(hw), offs1(hw);
      rs_pass(0, rs_plan(fb).bits, b.ka.p(), b.va.p(), k2.p(), v2.p(), pitch, 0, hist1.p(), offs1.p(), tiles, K, true);
      settle();
      const unsigned* r = sort_all(b, K, pitch, fb, true, nullptr);
      b.dump(out, r);
      k2.dump(out, false); v2.dump(out, false); hist1.dump(out, true); offs1.dump(out, true);
    } else {
      const unsigned* r = sort_all(b, K, pitch, fb, false, nullptr);
      b.dump(out, r);
    }
  }
}

static void case_points(Reader& in, FILE* out) {
  const int K = (int)in.one();
  const size_t pitch = in.one();
  const int cb = (int)in.one();
  REQ(K >= 1 && K <= 64 && pitch >= 1 && pitch <= (1u << 22) && cb >= 1 && cb <= 31);
  const size_t words = (size_t)K * pitch, hw = hist_words(K, pitch, cb);
  const unsigned* n = in.many((size_t)K);
  std::vector<GridDesc> gd((size_t)K);
  memset(gd.data(), 0, gd.size() * sizeof(GridDesc));
  for (int b = 0; b < K; b++) {
    const unsigned* g = in.many(7);
    for (int a = 0; a < 3; a++) gd[(size_t)b].min_b[a] = (int)g[a];
    gd[(size_t)b].mul1 = (int)g[3]; gd[(size_t)b].mul2 = (int)g[4];
    memcpy(&gd[(size_t)b].inv_leaf, &g[5], 4);
    gd[(size_t)b].status = (int)g[6];
    REQ(n[b] <= pitch);
  }
  const unsigned* pts = in.many(3 * words);
  const int tiles = (int)((pitch + RS_TILE - 1) / RS_TILE);
  Buf dpts(3 * words), dn((size_t)K), dgd(((size_t)K * sizeof(GridDesc) + 3) / 4);
  dpts.put(pts, 3 * words); dn.put(n, (size_t)K);
  CK(hipMemcpy(dgd.p(), gd.data(), gd.size() * sizeof(GridDesc), hipMemcpyHostToDevice));
  RsPoints src = {(const float*)dpts.p(), (const int*)dn.p(), (const GridDesc*)dgd.p(), cb, nullptr};
  {
    Buf k1(words), v1(words), k2(words), v2(words), hist1(hw), offs1(hw);
    src.keys = k1.p();
    rs_pass(0, rs_plan(cb).bits, k1.p(), v1.p(), k2.p(), v2.p(), pitch, 0, hist1.p(), offs1.p(), tiles, K, true, &src);
    settle();
    k1.dump(out, true); v1.dump(out, false); k2.dump(out, false); v2.dump(out, false); hist1.dump(out, true); offs1.dump(out, true);
  }
  SortBufs b(words, hw);
  src.keys = b.ka.p();
  const unsigned* r = sort_all(b, K, pitch, cb, true, &src);
  b.dump(out, r);
}

static void case_scan(Reader& in, FILE* out) {
  const unsigned kind = in.one();
  if (kind == 0) {
    const size_t n = in.one();
    REQ(n >= 1 && n <= (1u << 24));
    const int chunks = (int)((n + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK);
    Buf flag(n), tmp((size_t)chunks), pos(n);
    flag.put(in.many(n), n);
    k_pf_scan_totals<<<chunks, 1024>>>((const int*)flag.p(), n, tmp.p());
    k_pf_scan_offsets<<<1, 1024>>>(tmp.p(), chunks);
    k_pf_scan_apply<<<chunks, 1024>>>((const int*)flag.p(), n, tmp.p(), (int*)pos.p());
    settle();
    tmp.dump(out, true); pos.dump(out, true);
  } else if (kind == 1) {
    const int nchunks = (int)in.one();
    REQ(nchunks >= 1 && nchunks <= (1 << 20));
    Buf tot((size_t)nchunks);
    tot.put(in.many((size_t)nchunks), (size_t)nchunks);
    k_pf_scan_offsets<<<1, 1024>>>(tot.p(), nchunks);
    settle();
    tot.dump(out, true);
  } else {
    REQ(kind == 2);
    const int K = (int)in.one(), chunks = (int)in.one();
    const size_t rp = in.one();
    REQ(K >= 1 && K <= 64 && chunks >= 1 && rp >= 1 && (size_t)chunks == (rp + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK && rp <= (1u << 22));
    std::vector<PfbItem> items((size_t)K);
    for (int b = 0; b < K; b++) {
      const unsigned* w = in.many(3);
      items[(size_t)b] = PfbItem{nullptr, (unsigned long long)w[0], (int)w[1], (int)w[2]};
    }
    const size_t words = (size_t)K * rp;
    Buf ditems(((size_t)K * sizeof(PfbItem) + 3) / 4), flag(words), mm(6 * (size_t)K), res(PFB_RES_WORDS(K)), tmp((size_t)K * chunks), pos(words);
    CK(hipMemcpy(ditems.p(), items.data(), items.size() * sizeof(PfbItem), hipMemcpyHostToDevice));
    flag.put(in.many(words), words);
    k_pfb_begin<<<(6 * K + 255) / 256, 256>>>((int*)mm.p(), (int*)res.p(), K);
    k_pfb_scan_totals<<<xcd_grid(chunks, K), 1024>>>((const int*)flag.p(), rp, tmp.p(), chunks, K);
    k_pfb_scan_offsets<<<K, 1024>>>(tmp.p(), chunks, (const PfbItem*)ditems.p(), K, (int*)res.p());
    k_pfb_scan_apply<<<xcd_grid(chunks, K), 1024>>>((const int*)flag.p(), rp, tmp.p(), (int*)pos.p(), chunks, K);
    settle();
    mm.dump(out, false); res.dump(out, true); tmp.dump(out, true); pos.dump(out, true);
  }
}

static void case_heads(Reader& in, FILE* out) {
  const int K = (int)in.one();
  const size_t rp = in.one();
  const int downsample = (int)in.one();
  REQ(K >= 1 && K <= 64 && rp >= 1 && rp <= (1u << 22));
  std::vector<PfbItem> items((size_t)K);
  std::vector<PfGrid> grid((size_t)K);
  memset(grid.data(), 0, grid.size() * sizeof(PfGrid));
  for (int b = 0; b < K; b++) {
    const unsigned* w = in.many(2);
    REQ(w[0] <= rp);
    items[(size_t)b] = PfbItem{nullptr, 0ull, (int)w[0], b};
    grid[(size_t)b].status = (int)w[1];
  }
  const size_t words = (size_t)K * rp;
  const unsigned* keys = in.many(words);
  const unsigned* keepw = in.many(words);
  std::vector<unsigned char> keep((words + 3) / 4 * 4, 0);
  for (size_t i = 0; i < words; i++) keep[i] = (unsigned char)keepw[i];
  const int tiles = (int)((rp + RS_TILE - 1) / RS_TILE);
  Buf ditems(((size_t)K * sizeof(PfbItem) + 3) / 4), dgrid(((size_t)K * sizeof(PfGrid) + 3) / 4), dkeys(words), dkeep(keep.size() / 4), f1(words), f2(words);
  CK(hipMemcpy(ditems.p(), items.data(), items.size() * sizeof(PfbItem), hipMemcpyHostToDevice));
  CK(hipMemcpy(dgrid.p(), grid.data(), grid.size() * sizeof(PfGrid), hipMemcpyHostToDevice));
  Buf dgrid0(dgrid.n);                                                           // the same clouds, every grid usable
  CK(hipMemset(dgrid0.p(), 0, grid.size() * sizeof(PfGrid)));
  dkeys.put(keys, words);
  CK(hipMemcpy(dkeep.p(), keep.data(), keep.size(), hipMemcpyHostToDevice));
  const unsigned char* kp = (const unsigned char*)dkeep.p();
  k_pfb_heads<<<xcd_grid(tiles, K), 256>>>(dkeys.p(), kp, rp, (const PfbItem*)ditems.p(), K, tiles, (const PfGrid*)dgrid0.p(), downsample, (int*)f1.p());
  k_pfb_heads<<<xcd_grid(tiles, K), 256>>>(dkeys.p(), kp, rp, (const PfbItem*)ditems.p(), K, tiles, (const PfGrid*)dgrid.p(), downsample, (int*)f2.p());
  settle();
  f1.dump(out, true); f2.dump(out, true);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "plan")) {
    for (int f = 0; f <= 33; f++) { const RsPlan p = rs_plan(f); printf("%d %d %d\n", f, p.bits, p.passes); }
    return 0;
  }
  if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: %s plan | run <in.u32> <out.u32>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  fseek(f, 0, SEEK_END);
  const size_t nw = (size_t)ftell(f) / 4;
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned> a(nw);
  if (nw < 3 || fread(a.data(), 4, nw, f) != nw) { fprintf(stderr, "%s: short file\n", argv[2]); return 2; }
  fclose(f);
  Reader in{a.data(), nw};
  REQ(in.one() == 0x31435353u);
  const unsigned mode = in.one(), ncases = in.one();
  REQ(mode >= 1 && mode <= 4);
  FILE* out = fopen(argv[3], "wb");
  if (!out) { perror(argv[3]); return 2; }
  for (unsigned c = 0; c < ncases; c++) {
    if (mode == 1) case_sort(in, out);
    else if (mode == 2) case_points(in, out);
    else if (mode == 3) case_scan(in, out);
    else case_heads(in, out);
  }
  REQ(in.at == in.n);
  if (fclose(out) != 0) { perror(argv[3]); return 2; }
  return 0;
}
