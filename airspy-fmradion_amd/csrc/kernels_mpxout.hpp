// kernels_mpxout.hpp -- MPX output of an FM chain (fmr_enable_mpx_output): every stream's 384 kHz
// composite baseband, resampled to rate = 384000 L / M by a polyphase FIR, scaled and converted to S16 or F32 PCM into a
// ring of mono frames per stream.  A sibling of the output stage's rate converter (kernels_output.hpp, whose conversion
// rules OutSample and whose totals out_add_totals it uses), and a reader only: it takes the call's MPX where the RDS
// stage, the modulation monitor and the weak-signal detector take it, and writes nothing but its own ring, carry and
// totals.
//
// Launches per call with MPX samples, on the tail's stream:
//   k_mpx_rate  256 ring frames per workgroup, one per thread.  The workgroup stages the MPX span its frames reach -- at most
//               (255 M) / L + 1 + T samples, as the fp32 values they are -- into LDS: samples of this call from the call's
//               MPX row, the up to T - 1 samples in front of the call from the stage's carry.  Every thread then runs the
//               serial sum of the definition over its phase's taps, forming z = (double)x gain at use (the same bits as a
//               staged z in half the LDS), converts, stores at slot m mod max_frames, and the workgroup adds its clip /
//               non-finite counts to the stream's totals (butterfly, wave order, one integer atomic each).  Taps are read
//               from the prototype as it is, h[k L + p]: at a fixed k the lanes of a wave read within one row of L doubles
//               (one address for L = 1).  LDS reads: lane t reads float (q_t - k), q_t = floor(m_t M / L): consecutive lanes
//               are M / L words apart, a 2-way conflict of the 32-lane groups at 192000, 4-way at 96000, none worth a
//               transposed layout beside two fp64 operations per tap.
//   k_mpx_copy  rate 384000 (L = M = T = 1): acc = z[j], a plain convert-and-store, no LDS, no carry.
//   k_mpx_hist  the last T - 1 samples of [carry | call] to the other carry row, which the next call reads.  Two rows by
//               call parity: a call's k_mpx_rate reads row `par` while nothing writes it.
// Positions (first MPX sample, first ring frame, parity) live on the host and travel in MpxOutArgs, taken when the call is
// issued: the pipelined chain's tail runs a call behind.  Nothing here waits on another workgroup or on the host; there are
// no float atomics.  The translation unit is compiled with -ffp-contract=off: every product and sum is rounded by itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_output.hpp"

namespace fmr {

constexpr int kMpxThreads = kOutThreads;      // (out_add_totals joins a workgroup of that size)

struct MpxOutGeom {
  int L, M, T;               // rate / 384000 = L / M in lowest terms; taps per phase (L = M = T = 1: no filter)
  int span;                  // MPX samples a workgroup of k_mpx_rate stages at most: 255 M / L + 1 + T
};

struct MpxOutArgs {
  unsigned long long n0;     // MPX samples of the stream before this call
  unsigned long long n;      // MPX samples of the call
  unsigned long long out0;   // ring frames produced before this call: ceil(n0 L / M)
  unsigned long long n_out;  // ring frames of the call
  double gain;
  unsigned max_frames;
  int par;                   // the carry row that holds the T - 1 samples in front of this call (the other one gets the next ones)
};

// base: the call's MPX, sample j of stream s at base[s bstride + boff + (j - n0)]; carry [2][S][T - 1]; h: the prototype,
// T L doubles; ring [S][max_frames] samples; totals [S][2]: clipped, non-finite.
// Dynamic LDS: span floats, then 2 (kMpxThreads / 64) counters.
template <int FMT>
__global__ __launch_bounds__(kMpxThreads) void k_mpx_rate(const float *__restrict__ base, long long bstride, int boff,
                                                          const float *__restrict__ carry, const double *__restrict__ h,
                                                          MpxOutGeom gm, MpxOutArgs a, void *__restrict__ ring,
                                                          unsigned long long *__restrict__ totals) {
  using S = OutSample<FMT>;
  using V = typename S::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char mpx_lds[];
  float *xs = reinterpret_cast<float *>(mpx_lds);
  unsigned *s_cnt = reinterpret_cast<unsigned *>(mpx_lds + (size_t)gm.span * sizeof(float));
  const int s = blockIdx.y, hist = gm.T - 1;
  const unsigned long long uL = (unsigned long long)gm.L, uM = (unsigned long long)gm.M;
  const unsigned long long m_end = a.out0 + a.n_out;
  const unsigned long long m_first = a.out0 + (unsigned long long)blockIdx.x * kMpxThreads;     // (< m_end: the grid is ceil(n_out / 256))
  const unsigned long long m_last = min(m_first + (unsigned long long)(kMpxThreads - 1), m_end - 1);
  // n0 <= q_first <= q_last < n0 + n: m >= out0 = ceil(n0 L / M) gives m M >= n0 L, m < ceil((n0 + n) L / M) gives m M < (n0 + n) L
  const unsigned long long q_first = m_first * uM / uL, q_last = m_last * uM / uL;
  // the span is x[q_first - (T - 1)] .. x[q_last]; entry i is sample n0 + r, r = (q_first - n0) - (T - 1) + i >= -(T - 1)
  const int cnt = (int)(q_last - q_first) + gm.T;       // (<= span)
  const long long r0 = (long long)(q_first - a.n0) - hist;
  const float *row = base + (long long)s * bstride + boff;
  const float *crow = carry + ((long long)a.par * gridDim.y + s) * hist;
  for (int i = threadIdx.x; i < cnt; i += kMpxThreads) {
    const long long r = r0 + i;
    xs[i] = r >= 0 ? row[r] : crow[hist + r];
  }
  __syncthreads();
  const unsigned long long m = m_first + threadIdx.x;
  unsigned cl = 0, nf = 0;
  if (m <= m_last) {
    const unsigned long long mm = m * uM, q = mm / uL;
    const int p = (int)(mm - q * uL);
    const float *xq = xs + (int)(q - q_first) + hist;      // x[q]
    const double *hp = h + p;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < gm.T; k++) acc = acc + hp[(long long)k * gm.L] * ((double)xq[-k] * a.gain);
    const V v = S::conv(acc, cl, nf);
    // frames a later frame of this call lands on are not written: no two lanes ever write one slot
    const unsigned long long keep_from = a.n_out > a.max_frames ? m_end - a.max_frames : 0ull;
    if (m >= keep_from) (reinterpret_cast<V *>(ring) + (size_t)s * a.max_frames)[m % a.max_frames] = v;
  }
  out_add_totals(cl, nf, s_cnt, totals + 2 * s);
}

// rate 384000: ring frame m is sample m
template <int FMT>
__global__ __launch_bounds__(kMpxThreads) void k_mpx_copy(const float *__restrict__ base, long long bstride, int boff,
                                                          MpxOutArgs a, void *__restrict__ ring,
                                                          unsigned long long *__restrict__ totals) {
  using S = OutSample<FMT>;
  using V = typename S::type;
  __shared__ unsigned s_cnt[2 * (kMpxThreads / 64)];
  const int s = blockIdx.y;
  const unsigned long long r = (unsigned long long)blockIdx.x * kMpxThreads + threadIdx.x;
  unsigned cl = 0, nf = 0;
  if (r < a.n) {
    const V v = S::conv((double)base[(long long)s * bstride + boff + (long long)r] * a.gain, cl, nf);
    const unsigned long long m = a.n0 + r;
    const unsigned long long keep_from = a.n > a.max_frames ? a.n0 + a.n - a.max_frames : 0ull;
    if (m >= keep_from) (reinterpret_cast<V *>(ring) + (size_t)s * a.max_frames)[m % a.max_frames] = v;
  }
  out_add_totals(cl, nf, s_cnt, totals + 2 * s);
}

// carry row par ^ 1, entry i = sample n0 + n - (T - 1) + i: of this call where that is >= n0, else of row par
__global__ __launch_bounds__(kMpxThreads) void k_mpx_hist(const float *__restrict__ base, long long bstride, int boff,
                                                          float *__restrict__ carry, int hist, MpxOutArgs a) {
  const int i = blockIdx.x * kMpxThreads + threadIdx.x, s = blockIdx.y;
  if (i >= hist) return;
  const long long r = (long long)a.n - hist + i;      // (>= -hist)
  const float *src = carry + ((long long)a.par * gridDim.y + s) * hist;
  float *dst = carry + ((long long)(a.par ^ 1) * gridDim.y + s) * hist;
  dst[i] = r >= 0 ? base[(long long)s * bstride + boff + r] : src[hist + r];
}

}  // namespace fmr
