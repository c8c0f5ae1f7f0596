// Is v_mfma_f64_16x16x4_f64 a k-ordered chain of fused multiply-adds?
//   hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -o test_mfma_f64_chain tools/test_mfma_f64_chain.hip && ./test_mfma_f64_chain
// For random 16 x 4 and 4 x 16 operands of mixed magnitude (so that every order and every rounding scheme gives other
// bits) it counts, per output element, which host model the instruction's result equals:
//   asc   c -> fma(a[i][0], b[0][j], .) -> ... -> fma(a[i][3], b[3][j], .)      (what a banded FIR needs)
//   desc  the same chain with k descending
//   mul+add, k ascending, two roundings per tap
// and the same for two instructions chained through the accumulator (K = 8).  Also: a zero tap against a finite sample
// must leave the accumulator's bits alone (the zeros of a band), and against a NaN it must not (what to expect of a band
// over a non-finite sample).  Exit status 0 when every element equals `asc`.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

typedef double d4 __attribute__((ext_vector_type(4)));

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// one wave per trial: A [16][8], B [8][16], C [16][16] row-major; D1 after k = 0..3, D2 after k = 0..7
__global__ __launch_bounds__(64) void k_mfma(const double *A, const double *B, const double *C, double *D1, double *D2) {
  const int t = blockIdx.x, l = threadIdx.x, rc = l & 15, kq = l >> 4;
  A += t * 128; B += t * 128; C += t * 256; D1 += t * 256; D2 += t * 256;
  d4 acc;
  for (int r = 0; r < 4; r++) acc[r] = C[(kq + 4 * r) * 16 + rc];
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[rc * 8 + kq], B[kq * 16 + rc], acc, 0, 0, 0);
  for (int r = 0; r < 4; r++) D1[(kq + 4 * r) * 16 + rc] = acc[r];
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[rc * 8 + 4 + kq], B[(4 + kq) * 16 + rc], acc, 0, 0, 0);
  for (int r = 0; r < 4; r++) D2[(kq + 4 * r) * 16 + rc] = acc[r];
}

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main() {
  const int T = 512;
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::uniform_int_distribution<int> ex(-20, 20);
  std::vector<double> A(T * 128), B(T * 128), C(T * 256), D1(T * 256), D2(T * 256);
  for (auto &v : A) v = std::ldexp(u(rng), ex(rng));
  for (auto &v : B) v = std::ldexp(u(rng), ex(rng));
  for (auto &v : C) v = std::ldexp(u(rng), ex(rng));
  // trial 0: zero taps in k = 1, 2 (rows 0..7) -- trial 1: the same zeros against a NaN sample in B[1][3]
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 8; i++) { A[t * 128 + i * 8 + 1] = 0.0; A[t * 128 + i * 8 + 2] = 0.0; }
  B[1 * 128 + 1 * 16 + 3] = std::nan("");
  double *dA, *dB, *dC, *dD1, *dD2;
  CHK(hipMalloc(&dA, A.size() * 8)); CHK(hipMalloc(&dB, B.size() * 8)); CHK(hipMalloc(&dC, C.size() * 8));
  CHK(hipMalloc(&dD1, D1.size() * 8)); CHK(hipMalloc(&dD2, D2.size() * 8));
  CHK(hipMemcpy(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice));
  CHK(hipMemcpy(dB, B.data(), B.size() * 8, hipMemcpyHostToDevice));
  CHK(hipMemcpy(dC, C.data(), C.size() * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mfma, dim3(T), dim3(64), 0, 0, dA, dB, dC, dD1, dD2);
  CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(D1.data(), dD1, D1.size() * 8, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(D2.data(), dD2, D2.size() * 8, hipMemcpyDeviceToHost));
  long n = 0, asc[2] = {0, 0}, desc[2] = {0, 0}, unf[2] = {0, 0}, nan_rows = 0, nan_expected = 0;
  for (int t = 0; t < T; t++)
    for (int i = 0; i < 16; i++)
      for (int j = 0; j < 16; j++) {
        const double *a = &A[t * 128 + i * 8], *b = &B[t * 128 + j], c = C[t * 256 + i * 16 + j];
        for (int K = 4, w = 0; K <= 8; K += 4, w++) {
          const double got = (w ? D2 : D1)[t * 256 + i * 16 + j];
          double ra = c, ru = c, rd = c;
          for (int k = 0; k < K; k++) { ra = std::fma(a[k], b[k * 16], ra); ru = ru + a[k] * b[k * 16]; }
          for (int q = 0; q < K; q += 4)
            for (int k = q + 3; k >= q; k--) rd = std::fma(a[k], b[k * 16], rd);
          if (t == 1 && j == 3) { if (w == 0) { nan_rows += std::isnan(got); nan_expected += std::isnan(ra); } continue; }
          if (w == 0) n++;
          asc[w] += same(got, ra); desc[w] += same(got, rd); unf[w] += same(got, ru);
        }
      }
  printf("elements %ld\n", n);
  printf("one instruction  (K = 4): equal to asc-fma %ld  desc-fma %ld  asc mul+add %ld\n", asc[0], desc[0], unf[0]);
  printf("two instructions (K = 8): equal to asc-fma %ld  desc-fma %ld  asc mul+add %ld\n", asc[1], desc[1], unf[1]);
  printf("column with a NaN sample: NaN in %ld of 16 rows, the fma chain gives %ld\n", nan_rows, nan_expected);
  const bool ok = asc[0] == n && asc[1] == n;
  printf(ok ? "MFMA f64 == k-ascending fma chain\n" : "MFMA f64 is NOT the k-ascending fma chain\n");
  return ok ? 0 : 1;
}
