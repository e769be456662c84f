// TEST HELPER (tests/test_row_tree_gpu.py): the fixed-order reduction of a pair's partial rows (ndt_update.hpp: chunk_sum, group_sum,
// wave_sums_total, walk_groups, store_sums) on the device, alone, through the three forms the align routes use:
//   (a) the block form over four stored rows per chunk, plain loads           (k_update)
//   (b) the block form over chunk rows                                          (k_seq_update)
//   (c) the one-wave form, agent-scope loads, two groups in flight             (async_update)
// <in.f64>: [n_cases] [chunk count of every case] [the cases' rows, 4 x 44 doubles per chunk] [the cases' chunk rows, 44 doubles per chunk].
// <out.u64>: per case 3 x 44 words, forms a, b, c: the sums as store_sums leaves them in a PairState -- score, g[6], H[36] as doubles, hits
// as the (long long) it is stored as.  The comparison with the tree written out in numpy happens in the test.
//   build: as the library (see __graft_entry__.build_row_tree_check)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ndt_types.hpp"
#include "ndt_math.hpp"
#include "ndt_update.hpp"

__device__ void put_sums(const PairState& S, unsigned long long* o, const int lane) {
  if (lane == 0) o[0] = (unsigned long long)__double_as_longlong(S.score);
  else if (lane < 7) o[lane] = (unsigned long long)__double_as_longlong(S.g[lane - 1]);
  else if (lane < 43) o[lane] = (unsigned long long)__double_as_longlong(S.H[lane - 7]);
  else if (lane == 43) o[lane] = (unsigned long long)S.hits;
}

// one block per case, as k_update / k_seq_update run it
template <bool CHUNK_ROWS>
__global__ void __launch_bounds__(UPD_THREADS) k_tree_block(const double* __restrict__ rows, const int* __restrict__ nchunks, const size_t* __restrict__ off,
                                                            unsigned long long* out, const int form) {
  __shared__ double sm[UPD_WAVES][NACC];
  __shared__ PairState S;
  const int i = blockIdx.x;
  const double v = reduce_pair_rows<false>(rows + off[i] * (CHUNK_ROWS ? 1 : 4) * NACC, nchunks[i], true, sm, CHUNK_ROWS);
  if (threadIdx.x >= 64) return;
  store_sums(S, threadIdx.x, v, false, false, nullptr);
  wave_lds_sync();
  put_sums(S, out + ((size_t)i * 3 + form) * NACC, threadIdx.x);
}

// one wave per case, as async_update runs it
__global__ void __launch_bounds__(64) k_tree_wave(const double* __restrict__ rows, const int* __restrict__ nchunks, const size_t* __restrict__ off, unsigned long long* out) {
  __shared__ PairState S;
  const int i = blockIdx.x, lane = threadIdx.x;
  double aw[UPD_WAVES] = {0.0, 0.0, 0.0, 0.0};
  if (lane < NACC) walk_groups<4, true, 2, UPD_WAVES>(rows + off[i] * 4 * NACC + lane, nchunks[i], 0, 1, aw);
  store_sums(S, lane, wave_sums_total(aw[0], aw[1], aw[2], aw[3]), false, false, nullptr);
  wave_lds_sync();
  put_sums(S, out + ((size_t)i * 3 + 2) * NACC, lane);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 3; } } while (0)

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const size_t nd = (size_t)ftell(f) / sizeof(double);
  fseek(f, 0, SEEK_SET);
  std::vector<double> a(nd);
  if (nd < 1 || fread(a.data(), sizeof(double), nd, f) != nd) return 2;
  fclose(f);
  const size_t n = (size_t)a[0];
  if (n == 0 || n > 4096 || nd < 1 + n) { fprintf(stderr, "%zu cases in %zu doubles\n", n, nd); return 2; }
  std::vector<int> cnt(n);
  std::vector<size_t> off(n);
  size_t total = 0;
  for (size_t i = 0; i < n; i++) {
    if (!(a[1 + i] >= 0 && a[1 + i] <= 65536)) { fprintf(stderr, "case %zu: %g chunks\n", i, a[1 + i]); return 2; }
    cnt[i] = (int)a[1 + i]; off[i] = total; total += (size_t)cnt[i];
  }
  if (nd != 1 + n + total * 5 * NACC) { fprintf(stderr, "%zu doubles, expected %zu\n", nd, 1 + n + total * 5 * NACC); return 2; }
  const double* rows4 = a.data() + 1 + n;
  const double* rows1 = rows4 + total * 4 * NACC;
  double *d4 = nullptr, *d1 = nullptr;
  int* dcnt = nullptr;
  size_t* doff = nullptr;
  unsigned long long* dout = nullptr;
  const size_t n_out = n * 3 * NACC;
  CK(hipMalloc((void**)&d4, (total * 4 * NACC + 1) * sizeof(double)));
  CK(hipMalloc((void**)&d1, (total * NACC + 1) * sizeof(double)));
  CK(hipMalloc((void**)&dcnt, n * sizeof(int)));
  CK(hipMalloc((void**)&doff, n * sizeof(size_t)));
  CK(hipMalloc((void**)&dout, n_out * sizeof(unsigned long long)));
  CK(hipMemcpy(d4, rows4, total * 4 * NACC * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemcpy(d1, rows1, total * NACC * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemcpy(dcnt, cnt.data(), n * sizeof(int), hipMemcpyHostToDevice));
  CK(hipMemcpy(doff, off.data(), n * sizeof(size_t), hipMemcpyHostToDevice));
  CK(hipMemset(dout, 0xA5, n_out * sizeof(unsigned long long)));            // (a word no form wrote does not pass for a sum)
  k_tree_block<false><<<(unsigned)n, UPD_THREADS>>>(d4, dcnt, doff, dout, 0);
  CK(hipGetLastError());
  k_tree_block<true><<<(unsigned)n, UPD_THREADS>>>(d1, dcnt, doff, dout, 1);
  CK(hipGetLastError());
  k_tree_wave<<<(unsigned)n, 64>>>(d4, dcnt, doff, dout);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<unsigned long long> o(n_out);
  CK(hipMemcpy(o.data(), dout, n_out * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  const bool wrote = fwrite(o.data(), sizeof(unsigned long long), o.size(), f) == o.size();
  if (fclose(f) != 0 || !wrote) { perror(argv[2]); return 2; }
  CK(hipFree(d4)); CK(hipFree(d1)); CK(hipFree(dcnt)); CK(hipFree(doff)); CK(hipFree(dout));
  return 0;
}
