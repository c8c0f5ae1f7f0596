// kernels_output.hpp -- output stage of a decoder chain (fmr_enable_output): what the reference's
// stream loop does behind the decoder (main.cpp:950-1002) -- IF squelch, gain, PCM conversion, the IF / AF level meters.
//
// Two launches per call, behind everything that writes the call's audio:
//   k_out_pcm     one workgroup per (block, stream), one thread per frame: reads the block's audio once, takes the gate
//                 from the block's IF RMS, writes the gated and scaled frames to the stream's PCM ring (frame f at slot
//                 f mod max_frames; a thread stores its whole frame at once, the workgroup a contiguous run) and leaves
//                 the block's sums over the float32-narrowed audio and its clip / non-finite counts in a partial.
//   k_out_blocks  one wave per stream: 64 blocks per load, the two EMAs (if_level 0.75 / 0.25, audio_level 0.95 / 0.05)
//                 over the call's blocks in order on lane broadcasts from the carried state, one record per block with
//                 IF samples to the record ring; commits the carry.
//
// Sums: thread t of k_out_pcm adds the frames t, t + 256, ... of the block in that order, channel 0 before channel 1;
// the 64 lanes of a wave are joined by a butterfly (xor 32, 16, 8, 4, 2, 1), the four waves added in wave order.  fp64,
// no atomics: the same audio gives the same bits.  Positions (block, frame and record counters) live on the host and
// travel as arguments; the device carries the two levels only.  Nothing here waits on another workgroup or on the host.
// The translation unit is compiled with -ffp-contract=off: every product and sum is rounded by itself.
// A chain with fmr_set_output_rate adds the three launches of the rate converter at the end of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmr {

constexpr int kOutThreads = 256;

// fmr_output_block, field for field (the engine checks the sizes)
struct OutRec {
  uint64_t block, first_frame;
  uint32_t n_frames, channels;
  float if_rms, if_level, audio_mean, audio_rms, audio_level;
  uint32_t gate_open, n_clipped, n_nonfinite;
};

// what k_out_pcm leaves per (stream, block with audio)
struct OutPart {
  double sum, sumsq;
  unsigned clipped, nonfinite;
};

struct OutArgs {
  unsigned long long block0;     // absolute index of the call's first block
  unsigned long long frame0;     // ... of its first audio frame
  unsigned long long rec0;       // records written before this call
  unsigned long long n_frames;   // audio frames of the call
  unsigned long long n_recs;     // blocks of the call with IF samples
  double squelch, gain;
  unsigned max_frames, max_blocks;
  // rate converter (fmr_set_output_rate); all zero without it
  unsigned long long out0;       // ring frames produced before this call: ceil(frame0 L / M)
  unsigned long long n_out;      // ring frames of the call
  int zpar;                      // which of the two staging rows takes this call's z (the other one gets the next history)
};

template <int FMT> struct OutSample;
template <> struct OutSample<0> {       // S16: rint(y 32767) half-even, saturated; NaN -> 0
  using type = short;
  static __device__ __forceinline__ short conv(double y, unsigned &clipped, unsigned &nonfinite) {
    if (y != y) { nonfinite++; return 0; }
    if (y - y != 0.0) nonfinite++;      // +-Inf (also saturated and counted below)
    double r = rint(y * 32767.0);
    if (r > 32767.0) { r = 32767.0; clipped++; }
    else if (r < -32768.0) { r = -32768.0; clipped++; }
    return (short)(int)r;
  }
};
template <> struct OutSample<1> {       // F32: (float)y, passed through; |y| > 1 counted
  using type = float;
  static __device__ __forceinline__ float conv(double y, unsigned &clipped, unsigned &nonfinite) {
    if (y - y != 0.0) nonfinite++;      // NaN, +-Inf
    if (fabs(y) > 1.0) clipped++;
    return (float)y;
  }
};
template <class T, int CH> struct OutFrame;
template <> struct OutFrame<short, 1> { using type = short; static __device__ __forceinline__ type pack(const short *v) { return v[0]; } };
template <> struct OutFrame<short, 2> {
  using type = unsigned;
  static __device__ __forceinline__ type pack(const short *v) { return (unsigned)(unsigned short)v[0] | ((unsigned)(unsigned short)v[1] << 16); }
};
template <> struct OutFrame<float, 1> { using type = float; static __device__ __forceinline__ type pack(const float *v) { return v[0]; } };
template <> struct OutFrame<float, 2> { using type = float2; static __device__ __forceinline__ type pack(const float *v) { return make_float2(v[0], v[1]); } };

__device__ __forceinline__ double out_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned out_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

// A workgroup of kOutThreads adds its clip / non-finite counts to a stream's totals, totals[0] and totals[1]: butterfly per
// wave, the waves in order, one integer atomic each.  s_cnt: 2 (kOutThreads / 64) words of LDS.  (k_out_rate, kernels_mpxout.hpp)
__device__ __forceinline__ void out_add_totals(unsigned cl, unsigned nf, unsigned *s_cnt, unsigned long long *totals) {
  cl = out_wave_sum(cl); nf = out_wave_sum(nf);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_cnt[2 * w] = cl; s_cnt[2 * w + 1] = nf; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned t = 0;
#pragma unroll
    for (int k = 0; k < kOutThreads / 64; k++) t += s_cnt[2 * k + threadIdx.x];
    if (t) atomicAdd(&totals[threadIdx.x], (unsigned long long)t);
  }
}

// aud: the call's audio as the decoder wrote it (row s at s astride, frames interleaved); if_rms_blk [S][nb]: the IF RMS of
// every block of this call (k_stats); ring [S][max_frames] frames; part [S][nb]
template <int FMT, int CH>
__global__ __launch_bounds__(kOutThreads) void k_out_pcm(const double *__restrict__ aud, long long astride, BlockTab bt,
                                                         const float *__restrict__ if_rms_blk, OutArgs a,
                                                         void *__restrict__ ring, OutPart *__restrict__ part) {
  using S = OutSample<FMT>;
  using T = typename S::type;
  using F = OutFrame<T, CH>;
  __shared__ double s_sum[kOutThreads / 64], s_sq[kOutThreads / 64];
  __shared__ unsigned s_cl[kOutThreads / 64], s_nf[kOutThreads / 64];
  const int b = blockIdx.x, s = blockIdx.y;
  const int n = bt.au_len[b];
  if (n == 0) return;
  const int off = bt.au_off[b];
  const double g = ((double)if_rms_blk[(long long)s * bt.nb + b] >= a.squelch) ? a.gain : 0.0;
  const double *x = aud + (long long)s * astride + (long long)off * CH;
  const unsigned long long fb = a.frame0 + (unsigned long long)off;      // the block's first frame
  // frames a later frame of this call lands on are not written: no two lanes ever write one slot
  const unsigned long long keep_from = a.n_frames > a.max_frames ? a.frame0 + a.n_frames - a.max_frames : 0ull;
  const unsigned L = a.max_frames;
  const unsigned slot0 = (unsigned)(fb % L);
  typename F::type *row = reinterpret_cast<typename F::type *>(ring) + (size_t)s * L;
  double sum = 0.0, sq = 0.0;
  unsigned cl = 0, nf = 0;
  for (int i = threadIdx.x; i < n; i += kOutThreads) {
    T v[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const double xv = x[(long long)i * CH + c];
      const double xf = (double)(float)xv;
      sum += xf;
      sq += xf * xf;
      v[c] = S::conv(xv * g, cl, nf);
    }
    if (ring && fb + (unsigned long long)i >= keep_from) {      // (ring = nullptr: k_out_rate writes the ring)
      unsigned slot = slot0 + (unsigned)i % L;      // (slot0, i % L < L <= 2^26: no overflow)
      if (slot >= L) slot -= L;
      row[slot] = F::pack(v);
    }
  }
  sum = out_wave_sum(sum); sq = out_wave_sum(sq); cl = out_wave_sum(cl); nf = out_wave_sum(nf);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_sum[w] = sum; s_sq[w] = sq; s_cl[w] = cl; s_nf[w] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    OutPart p;
    p.sum = s_sum[0]; p.sumsq = s_sq[0]; p.clipped = s_cl[0]; p.nonfinite = s_nf[0];
#pragma unroll
    for (int k = 1; k < kOutThreads / 64; k++) { p.sum += s_sum[k]; p.sumsq += s_sq[k]; p.clipped += s_cl[k]; p.nonfinite += s_nf[k]; }
    part[(long long)s * bt.nb + b] = p;
  }
}

// state [S]: (if_level, audio_level); ring [S][max_blocks] records, record k at slot k mod max_blocks
__global__ __launch_bounds__(64) void k_out_blocks(BlockTab bt, const float *__restrict__ if_rms_blk,
                                                   const OutPart *__restrict__ part, OutArgs a, int ch,
                                                   float2 *__restrict__ state, OutRec *__restrict__ ring) {
  const int s = blockIdx.x, lane = threadIdx.x;
  float ifl = state[s].x, aul = state[s].y;
  unsigned long long rec = a.rec0;
  // (records a later record of this call lands on are not written)
  const unsigned long long keep_from = a.n_recs > a.max_blocks ? a.rec0 + a.n_recs - a.max_blocks : 0ull;
  for (int b0 = 0; b0 < bt.nb; b0 += 64) {
    const int b = min(b0 + lane, bt.nb - 1);
    const bool live = b0 + lane < bt.nb;
    const int n_if = live ? bt.if_len[b] : 0;
    const int n_au = n_if ? bt.au_len[b] : 0;
    const float r = n_if ? if_rms_blk[(long long)s * bt.nb + b] : 0.f;
    OutPart p{};
    if (n_au) p = part[(long long)s * bt.nb + b];
    const double n = (double)ch * (double)n_au;
    const float mean = n_au ? (float)(p.sum / n) : 0.f;
    const float rms = n_au ? (float)sqrt(p.sumsq / n) : 0.f;
    float my_ifl = 0.f, my_aul = 0.f;
    unsigned long long my_rec = 0;
    const int cnt = min(64, bt.nb - b0);
    for (int j = 0; j < cnt; j++) {
      if (__builtin_amdgcn_readlane(n_if, j) == 0) continue;
      ifl = (float)(0.75 * (double)ifl + 0.25 * (double)readlane_f(r, j));
      if (__builtin_amdgcn_readlane(n_au, j) != 0) aul = (float)(0.95 * (double)aul + 0.05 * (double)readlane_f(rms, j));
      if (lane == j) { my_ifl = ifl; my_aul = aul; my_rec = rec; }
      rec++;
    }
    if (n_if && my_rec >= keep_from) {
      OutRec o;
      o.block = a.block0 + (unsigned long long)b;
      o.first_frame = a.frame0 + (unsigned long long)bt.au_off[b];
      o.n_frames = (uint32_t)n_au; o.channels = (uint32_t)ch;
      o.if_rms = r; o.if_level = my_ifl; o.audio_mean = mean; o.audio_rms = rms; o.audio_level = my_aul;
      o.gate_open = ((double)r >= a.squelch) ? 1u : 0u;
      o.n_clipped = p.clipped; o.n_nonfinite = p.nonfinite;
      ring[(size_t)s * a.max_blocks + (size_t)(my_rec % a.max_blocks)] = o;
    }
  }
  if (lane == 0) state[s] = make_float2(ifl, aul);
}

// ---- rate converter (fmr_set_output_rate): PCM at rate = 48000 L / M and / or downmixed ----
// Three launches behind k_out_pcm (which then leaves the ring alone and still makes the partials of the records):
//   k_out_z     one workgroup per (block, stream): z = x g (or ((xL + xR) 0.5) g) as doubles into the call's staging row,
//               behind the T - 1 frames of history the row starts with.
//   k_out_rate  256 ring frames per workgroup, one per thread: the workgroup stages the z span its frames reach into LDS,
//               every thread runs the serial sum of the definition over its phase's taps (read from the prototype as it
//               is, h[k L + p]: at a fixed k the lanes of a wave read within one row of L doubles, for L = 1 one
//               address), converts, stores its whole frame at slot m mod max_frames, and the workgroup adds its clip /
//               non-finite counts to the stream's totals (butterfly, wave order, one integer atomic each).
//   k_out_hist  the last T - 1 frames of [history | z] to the head of the other staging row, which takes the next call.
// Positions (first input frame, first ring frame, which row) travel in OutArgs.
struct OutRateGeom {
  int L, M, T;               // rate / 48000 = L / M in lowest terms; taps per phase (L = M = T = 1: no filter, acc = z)
  int span;                  // frames of z a workgroup of k_out_rate stages at most: 255 M / L + 1 + T
  long long zstride;         // doubles per stream in a staging row: (T - 1 + the call's most frames) channels
  long long zrow;            // doubles per staging row: S zstride
};

template <int CH_IN, int CH_OUT>
__global__ __launch_bounds__(kOutThreads) void k_out_z(const double *__restrict__ aud, long long astride, BlockTab bt,
                                                       const float *__restrict__ if_rms_blk, OutArgs a, OutRateGeom gm,
                                                       double *__restrict__ z) {
  const int b = blockIdx.x, s = blockIdx.y;
  const int n = bt.au_len[b];
  if (n == 0) return;
  const int off = bt.au_off[b];
  const double g = ((double)if_rms_blk[(long long)s * bt.nb + b] >= a.squelch) ? a.gain : 0.0;
  const double *x = aud + (long long)s * astride + (long long)off * CH_IN;
  double *row = z + (long long)a.zpar * gm.zrow + (long long)s * gm.zstride + (long long)(gm.T - 1 + off) * CH_OUT;
  if (CH_IN == CH_OUT) {
    for (int j = threadIdx.x; j < n * CH_IN; j += kOutThreads) row[j] = x[j] * g;
  } else {
    for (int i = threadIdx.x; i < n; i += kOutThreads) row[i] = ((x[2 * i] + x[2 * i + 1]) * 0.5) * g;
  }
}

// z: the two staging rows; h: the prototype, T L doubles; ring [S][max_frames] frames; totals [S][2]: clipped, non-finite.
// Dynamic LDS: span CH doubles, then 2 (kOutThreads / 64) counters.
template <int FMT, int CH>
__global__ __launch_bounds__(kOutThreads) void k_out_rate(const double *__restrict__ z, const double *__restrict__ h,
                                                          OutRateGeom gm, OutArgs a, void *__restrict__ ring,
                                                          unsigned long long *__restrict__ totals) {
  using S = OutSample<FMT>;
  using V = typename S::type;
  using F = OutFrame<V, CH>;
  extern __shared__ __attribute__((aligned(16))) unsigned char out_lds[];
  double *zs = reinterpret_cast<double *>(out_lds);
  unsigned *s_cnt = reinterpret_cast<unsigned *>(out_lds + (size_t)gm.span * CH * sizeof(double));
  const int s = blockIdx.y;
  const unsigned long long uL = (unsigned long long)gm.L, uM = (unsigned long long)gm.M;
  const unsigned long long m_end = a.out0 + a.n_out;
  const unsigned long long m_first = a.out0 + (unsigned long long)blockIdx.x * kOutThreads;     // (< m_end: the grid is ceil(n_out / 256))
  const unsigned long long m_last = min(m_first + (unsigned long long)(kOutThreads - 1), m_end - 1);
  const unsigned long long q_first = m_first * uM / uL, q_last = m_last * uM / uL;
  // z[j] is frame T - 1 + (j - frame0) of the staging row; the span is z[q_first - (T - 1)] .. z[q_last]
  const int cnt = (int)(q_last - q_first) + gm.T;
  const double *src = z + (long long)a.zpar * gm.zrow + (long long)s * gm.zstride + (long long)(q_first - a.frame0) * CH;
  for (int j = threadIdx.x; j < cnt * CH; j += kOutThreads) zs[j] = src[j];
  __syncthreads();
  const unsigned long long m = m_first + threadIdx.x;
  unsigned cl = 0, nf = 0;
  if (m <= m_last) {
    const unsigned long long mm = m * uM, q = mm / uL;
    const int p = (int)(mm - q * uL);
    const double *zq = zs + ((long long)(q - q_first) + gm.T - 1) * CH;      // z[q]
    double acc[CH];
    if (gm.T == 1) {
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] = zq[c];
    } else {
#pragma unroll
      for (int c = 0; c < CH; c++) acc[c] = 0.0;
      const double *hp = h + p;
#pragma unroll 4
      for (int k = 0; k < gm.T; k++) {
        const double hk = hp[(long long)k * gm.L];
#pragma unroll
        for (int c = 0; c < CH; c++) acc[c] = acc[c] + hk * zq[-(long long)k * CH + c];
      }
    }
    V v[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) v[c] = S::conv(acc[c], cl, nf);
    // frames a later frame of this call lands on are not written: no two lanes ever write one slot
    const unsigned long long keep_from = a.n_out > a.max_frames ? m_end - a.max_frames : 0ull;
    if (m >= keep_from)
      (reinterpret_cast<typename F::type *>(ring) + (size_t)s * a.max_frames)[m % a.max_frames] = F::pack(v);
  }
  out_add_totals(cl, nf, s_cnt, totals + 2 * s);
}

// hist = (T - 1) channels doubles per stream, n = the call's frames times channels: from behind them in row zpar to the
// head of the other row
__global__ __launch_bounds__(kOutThreads) void k_out_hist(double *__restrict__ z, OutRateGeom gm, int zpar, long long n, int hist) {
  const int i = blockIdx.x * kOutThreads + threadIdx.x, s = blockIdx.y;
  if (i >= hist) return;
  const double *src = z + (long long)zpar * gm.zrow + (long long)s * gm.zstride + n;
  double *dst = z + (long long)(zpar ^ 1) * gm.zrow + (long long)s * gm.zstride;
  dst[i] = src[i];
}

}  // namespace fmr
