// kernels_mpxin.hpp -- MPX input of an FM chain (fmr_create_mpx_decoder): the front end of a chain that
// is fed composite baseband as mono S16 / F32 PCM at rate = 384000 L / M instead of IQ.  It produces what the discriminator
// produces on an IQ chain -- the call's MPX row (floats, at H_b + offset of `base`), its float copy d_dec (debug tap 1) and
// the per-block baseband sums -- and everything behind it (pilot PLL, audio tail, RDS stage, monitors, MPX output) runs as
// it does there.  The mirror image of kernels_mpxout.hpp: the same prototype filter, interpolating by M / L.
//
// Launches per call with frames, on the decoder stream:
//   k_mpx_in_rate   256 MPX samples per workgroup, one per thread.  The workgroup stages the frames its samples reach -- at
//                   most floor(255 L / M) + 1 + K, K = ceil(T L / M) -- into LDS: frames of this call from the call's PCM row,
//                   the up to K - 1 frames in front of the call from the stage's carry.  They are staged as z = u g' in fp64
//                   (converted once per frame, not once per tap; the bits of a z formed at use are the same, and 8 bytes x
//                   400 frames of LDS are nothing).  The S16 conversion v / 32767.0 is read from a table of the 65536
//                   quotients the host formed with that one fp64 division: the device's own division is a sequence of
//                   fused multiply-adds, and these kernels hold none.  Every thread then runs the
//                   serial sum of the definition, acc = acc + h[p + k M] z[i0 - k], k ascending.  The taps are the prototype
//                   as it is, padded with zeros to K M doubles so that every lane runs K terms: a padded term adds +-0.0 to
//                   an acc that is never -0.0 (it starts at +0.0, and z is finite: a non-finite frame was replaced by +0.0),
//                   which leaves every bit where the definition's shorter loop leaves it.  At a fixed k the lanes of a wave
//                   read within one row of M doubles.  LDS reads: lane t reads double (i0_t - k), i0_t = floor(j_t L / M):
//                   consecutive lanes are L / M <= 1 doubles apart -- neighbours share an address (broadcast) or sit in
//                   adjacent 8-byte slots: no bank conflict at any rate.
//                   Non-finite F32 frames are counted by the workgroup that stages them first (each frame of a call is new
//                   to exactly one workgroup): butterfly per wave, one integer atomicAdd per workgroup.
//   k_mpx_in_copy   rate 384000 (L = M = T = K = 1): x[j] = (float)(u[j] gain), convert and store, no LDS, no carry.
//   k_mpx_in_hist   the last K - 1 frames of [carry | call], as u, to the other carry row, which the next call reads.  Two
//                   rows by call parity, as in k_mpx_hist: a call's k_mpx_in_rate reads row `par` while nothing writes it.
//   k_mpx_in_stats  grid (blocks, streams): per-block mean and RMS of the MPX in k_disc's order -- lane t of 256 adds samples
//                   t, t + 256, ... ascending in fp32, d d as its own product, then block_sum<256> -- so that they are the
//                   bits a k_disc chain reports on the same MPX; and the block's IF RMS, 0: there is no IF.
// Positions (first frame, first MPX sample, parity) live on the host and travel in MpxInArgs.  Nothing here waits on another
// workgroup or on the host; there are no float atomics.  The translation unit is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "kernels_output.hpp"

namespace fmr {

constexpr int kMpxInThreads = 256;

struct MpxInGeom {
  int L, M, T, K;            // rate / 384000 = L / M in lowest terms; taps per phase of the prototype; terms per sample, ceil(T L / M)
  int span;                  // frames a workgroup of k_mpx_in_rate stages at most: floor(255 L / M) + 1 + K
};

struct MpxInArgs {
  unsigned long long f0, nf; // frames of the stream before this call, frames of the call
  unsigned long long j0, n;  // MPX samples before this call: ceil(f0 M / L); MPX samples of the call
  double g;                  // gain (M / L), formed once on the host (gain itself at 384000)
  int par;                   // the carry row that holds the K - 1 frames in front of this call
};

// One PCM frame as u (include/fmradion_amd.h): S16 v / 32767.0, one fp64 division -- made on the host for every v, s16[v + 32768];
// F32 (double)v, a non-finite value +0.0 and counted.
template <int FMT> struct MpxInSample;
template <> struct MpxInSample<0> {
  using type = int16_t;
  static __device__ __forceinline__ double conv(int16_t v, const double *__restrict__ s16, unsigned &) { return s16[(int)v + 32768]; }
};
template <> struct MpxInSample<1> {
  using type = float;
  static __device__ __forceinline__ double conv(float v, const double *__restrict__, unsigned &nf) {
    if (v - v != 0.f) { nf++; return 0.0; }      // NaN, +-Inf
    return (double)v;
  }
};

// a workgroup adds its count to the stream's total: butterfly per wave, the waves in order, one integer atomic
__device__ __forceinline__ void mpx_in_add_total(unsigned nf, unsigned *s_cnt /* kMpxInThreads / 64 */, unsigned long long *total) {
  nf = out_wave_sum(nf);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = nf;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0;
#pragma unroll
    for (int k = 0; k < kMpxInThreads / 64; k++) t += s_cnt[k];
    if (t) atomicAdd(total, (unsigned long long)t);
  }
}

// pcm: the call's frames, frame f0 + r of stream s at pcm[s pstride + r]; carry [2][S][K - 1] doubles (u); h: the prototype
// padded to K M doubles; base / dec: the call's MPX, sample j0 + r of stream s at base[s bstride + boff + r] and
// dec[s dstride + r]; totals [S]: non-finite frames; s16: the 65536 quotients of the S16 conversion (F32: unused).
// Dynamic LDS: span doubles, then kMpxInThreads / 64 counters.
template <int FMT>
__global__ __launch_bounds__(kMpxInThreads) void k_mpx_in_rate(const void *__restrict__ pcm, long long pstride,
                                                               const double *__restrict__ s16, const double *__restrict__ carry,
                                                               const double *__restrict__ h,
                                                               MpxInGeom gm, MpxInArgs a, float *__restrict__ base, long long bstride,
                                                               int boff, float *__restrict__ dec, long long dstride,
                                                               unsigned long long *__restrict__ totals) {
  using P = MpxInSample<FMT>;
  using V = typename P::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char mpxin_lds[];
  double *zs = reinterpret_cast<double *>(mpxin_lds);
  unsigned *s_cnt = reinterpret_cast<unsigned *>(mpxin_lds + (size_t)gm.span * sizeof(double));
  const int s = blockIdx.y, hist = gm.K - 1;
  const unsigned long long uL = (unsigned long long)gm.L, uM = (unsigned long long)gm.M;
  const unsigned long long j_first = a.j0 + (unsigned long long)blockIdx.x * kMpxInThreads;      // (< j0 + n: the grid is ceil(n / 256))
  const unsigned long long j_last = min(j_first + (unsigned long long)(kMpxInThreads - 1), a.j0 + a.n - 1);
  // f0 <= i_first <= i_last < f0 + nf: j >= j0 = ceil(f0 M / L) gives j L >= f0 M, j < ceil((f0 + nf) M / L) gives j L < (f0 + nf) M
  const unsigned long long i_first = j_first * uL / uM, i_last = j_last * uL / uM;
  // the span is frames i_first - (K - 1) .. i_last; entry e is frame f0 + r, r = (i_first - f0) - (K - 1) + e >= -(K - 1)
  const int cnt = (int)(i_last - i_first) + gm.K;       // (<= span: i_last - i_first <= floor(255 L / M) + 1)
  const long long r0 = (long long)(i_first - a.f0) - hist;
  // frames new to this workgroup (counted here): behind the last frame the workgroup before it reached.  Consecutive samples
  // reach the same frame or the next one (L <= M), and the call's first sample reaches frame f0: no frame is left out.
  const long long own_lo = blockIdx.x == 0 ? 0ll : (long long)((j_first - 1) * uL / uM - a.f0) + 1;
  const V *row = reinterpret_cast<const V *>(pcm) + (long long)s * pstride;
  const double *crow = carry + ((long long)a.par * gridDim.y + s) * hist;
  unsigned nf = 0;
  for (int e = threadIdx.x; e < cnt; e += kMpxInThreads) {
    const long long r = r0 + e;
    double u;
    if (r >= 0) {
      unsigned c = 0;
      u = P::conv(row[r], s16, c);
      if (r >= own_lo) nf += c;
    } else {
      u = crow[hist + r];
    }
    zs[e] = u * a.g;
  }
  __syncthreads();
  const unsigned long long j = j_first + threadIdx.x;
  if (j <= j_last) {
    const unsigned long long jj = j * uL, i0 = jj / uM;
    const int p = (int)(jj - i0 * uM);
    const double *zq = zs + (int)(i0 - i_first) + hist;      // z[i0]
    const double *hp = h + p;
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < gm.K; k++) acc = acc + hp[(long long)k * gm.M] * zq[-k];
    const float x = (float)acc;
    const long long r = (long long)(j - a.j0);
    base[(long long)s * bstride + boff + r] = x;
    dec[(long long)s * dstride + r] = x;
  }
  mpx_in_add_total(nf, s_cnt, totals + s);
}

// rate 384000: MPX sample j is frame j
template <int FMT>
__global__ __launch_bounds__(kMpxInThreads) void k_mpx_in_copy(const void *__restrict__ pcm, long long pstride,
                                                               const double *__restrict__ s16, MpxInArgs a,
                                                               float *__restrict__ base, long long bstride, int boff,
                                                               float *__restrict__ dec, long long dstride,
                                                               unsigned long long *__restrict__ totals) {
  using P = MpxInSample<FMT>;
  using V = typename P::type;
  __shared__ unsigned s_cnt[kMpxInThreads / 64];
  const int s = blockIdx.y;
  const unsigned long long r = (unsigned long long)blockIdx.x * kMpxInThreads + threadIdx.x;
  unsigned nf = 0;
  if (r < a.n) {
    const double u = P::conv((reinterpret_cast<const V *>(pcm) + (long long)s * pstride)[r], s16, nf);
    const float x = (float)(u * a.g);
    base[(long long)s * bstride + boff + (long long)r] = x;
    dec[(long long)s * dstride + (long long)r] = x;
  }
  mpx_in_add_total(nf, s_cnt, totals + s);
}

// carry row par ^ 1, entry i = frame f0 + nf - (K - 1) + i as u: of this call where that is >= f0, else of row par.
// A non-finite frame is stored as the +0.0 it counted as (k_mpx_in_rate / k_mpx_in_copy did the counting).
template <int FMT>
__global__ __launch_bounds__(kMpxInThreads) void k_mpx_in_hist(const void *__restrict__ pcm, long long pstride,
                                                               const double *__restrict__ s16, double *__restrict__ carry, int hist, MpxInArgs a) {
  using P = MpxInSample<FMT>;
  using V = typename P::type;
  const int i = blockIdx.x * kMpxInThreads + threadIdx.x, s = blockIdx.y;
  if (i >= hist) return;
  const long long r = (long long)a.nf - hist + i;      // (>= -hist)
  const double *src = carry + ((long long)a.par * gridDim.y + s) * hist;
  double *dst = carry + ((long long)(a.par ^ 1) * gridDim.y + s) * hist;
  unsigned c = 0;
  dst[i] = r >= 0 ? P::conv((reinterpret_cast<const V *>(pcm) + (long long)s * pstride)[r], s16, c) : src[hist + r];
}

// per-block baseband mean / RMS of the call's MPX, the sums in k_disc's order (kernels.hpp), and the IF RMS of a chain
// without an IF
__global__ __launch_bounds__(kMpxInThreads) void k_mpx_in_stats(const float *__restrict__ base, long long bstride, int boff,
                                                                BlockTab bt, float *__restrict__ bb_mean_blk,
                                                                float *__restrict__ bb_rms_blk, float *__restrict__ if_rms_blk) {
  __shared__ float scratch[kMpxInThreads / 64];
  const int b = blockIdx.x, s = blockIdx.y;
  const int n = bt.if_len[b];
  if (n == 0) return;
  const float *x = base + (long long)s * bstride + boff + bt.if_off[b];
  float vsum = 0.f, vsq = 0.f;
  for (int i = threadIdx.x; i < n; i += kMpxInThreads) {
    const float d = x[i];
    vsum += d;
    vsq += d * d;
  }
  const float ts = block_sum<kMpxInThreads>(vsum, scratch);
  const float tq = block_sum<kMpxInThreads>(vsq, scratch);
  if (threadIdx.x == 0) {
    bb_mean_blk[(long long)s * bt.nb + b] = ts / (float)(unsigned)n;
    bb_rms_blk[(long long)s * bt.nb + b] = sqrtf(tq / (float)(unsigned)n);
    if_rms_blk[(long long)s * bt.nb + b] = 0.f;
  }
}

}  // namespace fmr
