// TEST HELPER (tests/test_build_stages_gpu.py): the two kernels of the target build (ndt_build.hpp) that point clouds cannot steer -- k_voxels on
// synthetic sums and counts, and k_build_check, which only the stream's planned builds launch -- on the device, alone.  It launches the library's
// own kernels and restates neither; every comparison happens in the test, against mpmath and plain arithmetic.
//
//   build_check run <in.u32> <out.u32>    runs every case of the file
//
// <in.u32>, 32-bit little-endian words: [0x31434C42] [mode] [number of cases], then the cases one after the other.
//   mode 1, voxels:  [n_voxels] [cap] [pca] [opt] [eig_mult: f64, two words] sums[n_voxels * 9] (f64, two words each) counts[n_voxels]
//     One target at rec_off 0 with room for cap >= n_voxels records; opt bit 0: icov64, bit 1: kd_weight, bit 2: recs_fast (else a null pointer).
//     Launched as the build launches it: one thread per record slot, dim3(ceil(cap / 256), 1) blocks of 256.
//     out: RECS (cap * 16 words) VOX_N (cap; the counts in front, 0xA5 behind) ICOV64 (cap * 18) KD_WEIGHT (cap) RECS_FAST (cap * 16)
//   mode 2, check:   [n_pairs] [plan_words] [plan_cb] [total words] [largest grid] n_pairs x {status ncells nwords word_off n_voxels} nwords[n_pairs]
//     k_build_check as the planned build launches it: ceil(n_pairs / 256) blocks of 256.
//     out: STAT (3 words) GRIDDESC (n_pairs * 19 words) NWORDS (n_pairs)
// <out.u32>: the output buffers of every case in the order above, each as [n] [64 guard words] [n words] [64 guard words]; a buffer the case did
// not ask for has n = 0 (its guard words only).  Every buffer is filled with 0xA5A5A5A5, guards included, before the launch: a word the kernel
// did not write, or wrote outside its buffer, shows in the test.
//   build: as the library (see __graft_entry__.build_build_check)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ndt_types.hpp"
#include "ndt_math.hpp"
#include "ndt_build.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(3); } } while (0)
#define REQ(c) do { if (!(c)) { fprintf(stderr, "bad case file: %s (line %d)\n", #c, __LINE__); exit(2); } } while (0)
#define GUARD 64
static_assert(sizeof(GridDesc) == 19 * 4 && sizeof(VoxelRec) == 64 && sizeof(VoxelRecF) == 64, "the layouts the test decodes");

// a device buffer of n words between two rows of guard words (8-byte aligned: GUARD is even)
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
  void put(const void* src, size_t words) const { if (words) CK(hipMemcpy(p(), src, words * sizeof(unsigned), hipMemcpyHostToDevice)); }
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

static void case_voxels(Reader& in, FILE* out) {
  const size_t nv = in.one(), cap = in.one();
  const int pca = (int)in.one();
  const unsigned opt = in.one();
  double eig_mult;
  memcpy(&eig_mult, in.many(2), 8);
  REQ(nv >= 1 && nv <= cap && cap <= (1u << 16) && pca <= 1 && opt <= 7);
  const unsigned* sums = in.many(nv * 18);
  const unsigned* counts = in.many(nv);
  GridDesc g;
  memset(&g, 0, sizeof g);
  g.n_voxels = (int)nv;                                                          // rec_off 0: the one target of this launch
  Buf dgd(19), dsums(cap * 18), recs(cap * 16), vox_n(cap), icov64(cap * 18), kdw(cap), fast(cap * 16);
  dgd.put(&g, 19); dsums.put(sums, nv * 18); vox_n.put(counts, nv);
  k_voxels<<<dim3((unsigned)((cap + 255) / 256), 1), 256>>>((const GridDesc*)dgd.p(), (const double*)dsums.p(), (VoxelRec*)recs.p(), (int*)vox_n.p(), eig_mult, pca,
                                                            (opt & 1) ? (double*)icov64.p() : nullptr, (opt & 2) ? (int*)kdw.p() : nullptr,
                                                            (opt & 4) ? (VoxelRecF*)fast.p() : nullptr);
  settle();
  recs.dump(out, true); vox_n.dump(out, true); icov64.dump(out, opt & 1); kdw.dump(out, opt & 2); fast.dump(out, opt & 4);
}

static void case_check(Reader& in, FILE* out) {
  const int B = (int)in.one();
  const unsigned plan_words = in.one();
  const int plan_cb = (int)in.one();
  const unsigned info[2] = {in.one(), in.one()};
  REQ(B >= 1 && B <= (1 << 16) && plan_cb >= 1 && plan_cb <= 32);
  std::vector<GridDesc> gd((size_t)B);
  memset(gd.data(), 0, gd.size() * sizeof(GridDesc));
  for (int b = 0; b < B; b++) {
    const unsigned* w = in.many(5);
    gd[(size_t)b].status = (int)w[0]; gd[(size_t)b].ncells = (int)w[1]; gd[(size_t)b].nwords = (int)w[2]; gd[(size_t)b].word_off = w[3]; gd[(size_t)b].n_voxels = (int)w[4];
    gd[(size_t)b].rec_off = 7u * (unsigned)b; gd[(size_t)b].mul1 = b + 1;          // fields the kernel has to leave alone
  }
  Buf dinfo(2), dgd((size_t)B * 19), dnw((size_t)B), stat(3);
  dinfo.put(info, 2); dgd.put(gd.data(), (size_t)B * 19); dnw.put(in.many((size_t)B), (size_t)B);
  k_build_check<<<(B + 255) / 256, 256>>>(dinfo.p(), (GridDesc*)dgd.p(), dnw.p(), B, plan_words, plan_cb, stat.p());
  settle();
  stat.dump(out, true); dgd.dump(out, true); dnw.dump(out, true);
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: %s run <in.u32> <out.u32>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[2], "rb");
  if (!f) { perror(argv[2]); return 2; }
  fseek(f, 0, SEEK_END);
  const size_t nw = (size_t)ftell(f) / 4;
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned> a(nw);
  if (nw < 3 || fread(a.data(), 4, nw, f) != nw) { fprintf(stderr, "%s: short file\n", argv[2]); return 2; }
  fclose(f);
  Reader in{a.data(), nw};
  REQ(in.one() == 0x31434C42u);
  const unsigned mode = in.one(), ncases = in.one();
  REQ(mode >= 1 && mode <= 2);
  FILE* out = fopen(argv[3], "wb");
  if (!out) { perror(argv[3]); return 2; }
  for (unsigned c = 0; c < ncases; c++) {
    if (mode == 1) case_voxels(in, out);
    else case_check(in, out);
  }
  REQ(in.at == in.n);
  if (fclose(out) != 0) { perror(argv[3]); return 2; }
  return 0;
}
