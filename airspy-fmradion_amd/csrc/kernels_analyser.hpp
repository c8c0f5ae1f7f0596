// kernels_analyser.hpp -- audio analyser of the decoded audio (fmr_enable_analyser).
//
// An instance of the Welch segment engine (kernels_welch.hpp: indices, the partition into sub-blocks and runs, the carry,
// the open records and the ring), counted in audio frames (one sample per channel), with N = fft_size (1024 .. 8192),
// H = N / 2, M = interval_samples and sub-blocks of 1 .. 16 segments.  What is this stage's own:
//
// k_an_seg<LOGN>: one workgroup = one run.  Per segment: N frames of fp64 audio from the call or the carry (frame p at
// p mod N), each sample rounded once to fp32 and multiplied by the fp32 window, z[n] = wL[n] + i wR[n] stored bit-reversed
// into padded LDS, then welch_fft.  With X = Z[k] and Y = conj Z[(N - k) mod N]:
// L[k] = (X + Y) / 2, R[k] = (X - Y) / (2 i) in fp32; |L|^2, |R|^2 and Re(L conj R) are formed in fp64 from those fp32
// values and folded into fp64 registers across the run, k = 0 .. N / 2.  With one channel the imaginary input is 0, the
// first row is |Z[k]|^2 and the other two stay 0.  A segment that holds a sample which is not finite as fp32 is skipped
// for the spectral part and counted.  The time-domain part of a record (sum, sum of squares, non-finite count) is taken
// over the FIRST H frames of each of its segments, so every frame enters it exactly once wherever a call ends; it takes a
// skipped segment's finite samples as they are and the others as 0.  One partial per run.
//
// k_an_reduce: the engine's reduce over the three rows of sums and AnRec; in the call's last launch it also copies the
// call's last N - 1 frames into the carry.
//
// The scaling to power, c_k / (N sum w^2 segments), happens on the host when a record is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_welch.hpp"

namespace fmr {

constexpr int kAnLogMin = 10, kAnLogMax = 13;
constexpr int kAnRows = 3;           // |L|^2, |R|^2, Re(L conj R)
constexpr int kAnRT = 256;           // threads of k_an_reduce
constexpr int kAnMaxRuns = 128;      // runs per stream and launch at most

template <int LOGN>
struct AnShape {
  static constexpr int N = 1 << LOGN, H = N / 2, NB = N / 2 + 1;
  static constexpr int T = N / 4 < 512 ? N / 4 : 512;        // threads: at least one radix-4 butterfly each per pass (512: 256 VGPRs each)
  static constexpr int SPT = N / T;                          // frames a thread loads per segment
  static constexpr int BPT = H / T;                          // bins a thread folds (thread 0: bin N / 2 as well)
  static constexpr int LDS_BYTES = (N + (N >> 5)) * 8;
};

// fmr_analyser_record, field for field (the engine checks the sizes)
struct AnRec {
  uint64_t index, first_sample;
  uint32_t segments, skipped, n_nonfinite, channels, fft_size, interval_samples;
  double sum[2], sumsq[2];
};

// what k_an_seg leaves per run beside its three rows of bins
struct AnPart {
  double sum[2], sumsq[2];
  unsigned segments, skipped, nnon, pad;
};

struct AnArgs : WelchArgs {
  int ch;              // channels (1 or 2: the audio is interleaved)
};

// bin k of the finished transform in lds into the three sums (pl, pr, pc): the conjugate-symmetric split for two
// channels, |Z[k]|^2 for one
template <int LOGN>
__device__ __forceinline__ void an_fold(const float2 *lds, int k, int ch, double &pl, double &pr, double &pc) {
  constexpr int N = AnShape<LOGN>::N;
  const float2 x = lds[spec_pad(k)];
  if (ch == 2) {
    const float2 z = lds[spec_pad((N - k) & (N - 1))];
    const double lr = (double)(0.5f * (x.x + z.x)), li = (double)(0.5f * (x.y - z.y));
    const double rr = (double)(0.5f * (x.y + z.y)), ri = (double)(-0.5f * (x.x - z.x));
    pl += lr * lr + li * li;
    pr += rr * rr + ri * ri;
    pc += lr * rr + li * ri;
  } else {
    pl += (double)x.x * (double)x.x + (double)x.y * (double)x.y;
  }
}

// Workgroup = (run r = blockIdx.x of the launch, stream s = blockIdx.y).  The call's audio of stream s at aud + s astride
// (frame n0 first, a.ch doubles per frame), the carry at carry + s N 2 (frame p at slot p mod N, two doubles per slot).
// Partials of the run at row s rmax + r: ppsd [kAnRows][N / 2 + 1], ppart.
template <int LOGN>
__global__ __launch_bounds__(AnShape<LOGN>::T) void k_an_seg(const double *__restrict__ aud, long long astride,
                                                             const double *__restrict__ carry, AnArgs a,
                                                             const float *__restrict__ win, const float2 *__restrict__ tw,
                                                             int rmax, double *__restrict__ ppsd, AnPart *__restrict__ ppart) {
  using S = AnShape<LOGN>;
  constexpr int N = S::N, H = S::H, NB = S::NB, T = S::T, SPT = S::SPT, BPT = S::BPT;
  extern __shared__ float2 lds_an[];
  const int tid = threadIdx.x, run = blockIdx.x, s = blockIdx.y, ch = a.ch;
  long long lo, hi;
  welch_sub(a.spr, a.sub, a.sb, a.g0 + run, lo, hi);
  const long long j_lo = lo > a.a0 ? lo : a.a0, j_hi = hi < a.a1 ? hi : a.a1;
  const double *x = aud + (long long)s * astride;
  const double *cr = carry + (long long)s * N * 2;

  double al[BPT], ar[BPT], ac[BPT];
#pragma unroll
  for (int b = 0; b < BPT; b++) { al[b] = 0.0; ar[b] = 0.0; ac[b] = 0.0; }
  double el = 0.0, er = 0.0, ec = 0.0;             // bin N / 2 (thread 0)
  double sum0 = 0.0, sum1 = 0.0, sq0 = 0.0, sq1 = 0.0;
  unsigned nnon = 0, counted = 0, skipped = 0;

  for (long long j = j_lo; j < j_hi; j++) {
    const long long p0 = j * H;
    int bad = 0;
#pragma unroll
    for (int q = 0; q < SPT; q++) {
      const int i = tid + q * T;
      const long long p = p0 + i;
      double vl, vr = 0.0;
      if (p >= a.n0) {
        const double *f = x + (p - a.n0) * ch;
        vl = f[0];
        if (ch == 2) vr = f[1];
      } else {
        const double *f = cr + (p & (N - 1)) * 2;
        vl = f[0]; vr = f[1];
      }
      if (q < SPT / 2) {                           // the segment's first H frames: the time-domain part
        const bool fl = isfinite(vl), fr = isfinite(vr);
        const double cl = fl ? vl : 0.0, cq = fr ? vr : 0.0;
        sum0 += cl; sq0 += cl * cl;
        sum1 += cq; sq1 += cq * cq;
        nnon += (unsigned)!fl + (unsigned)!fr;
      }
      const float gl = (float)vl, gr = (float)vr;
      bad |= !(isfinite(gl) && isfinite(gr));
      const float w = win[i];
      lds_an[spec_pad((int)(__brev((unsigned)i) >> (32 - LOGN)))] = make_float2(gl * w, gr * w);
    }
    bad = __syncthreads_or(bad);
    if (bad) { skipped++; continue; }              // (uniform: nobody has read the LDS, the next segment's stores may follow)
    welch_fft<LOGN, T>(lds_an, tw, tid);
#pragma unroll
    for (int b = 0; b < BPT; b++) an_fold<LOGN>(lds_an, tid + b * T, ch, al[b], ar[b], ac[b]);
    if (tid == 0) an_fold<LOGN>(lds_an, N / 2, ch, el, er, ec);
    counted++;
    __syncthreads();                               // every thread has read its bins before the next segment's stores
  }

  // the run's time-domain values: a fixed tree over the threads, two values at a time (the FFT's LDS is free now)
  __syncthreads();
  double *r_a = reinterpret_cast<double *>(lds_an), *r_b = r_a + T;      // 16 T bytes of the LDS's 33 T or more
  auto tree = [&](double &u, double &v) {
    r_a[tid] = u; r_b[tid] = v;
    __syncthreads();
    for (int st = T / 2; st > 0; st >>= 1) {
      if (tid < st) { r_a[tid] += r_a[tid + st]; r_b[tid] += r_b[tid + st]; }
      __syncthreads();
    }
    u = r_a[0]; v = r_b[0];
    __syncthreads();
  };
  tree(sum0, sum1);
  tree(sq0, sq1);
  unsigned *r_n = reinterpret_cast<unsigned *>(lds_an);
  r_n[tid] = nnon;
  __syncthreads();
  for (int st = T / 2; st > 0; st >>= 1) {
    if (tid < st) r_n[tid] += r_n[tid + st];
    __syncthreads();
  }
  const size_t prow = (size_t)s * rmax + run;
  double *out = ppsd + prow * (size_t)(kAnRows * NB);
#pragma unroll
  for (int b = 0; b < BPT; b++) {
    out[tid + b * T] = al[b];
    out[NB + tid + b * T] = ar[b];
    out[2 * NB + tid + b * T] = ac[b];
  }
  if (tid == 0) {
    out[N / 2] = el; out[NB + N / 2] = er; out[2 * NB + N / 2] = ec;
    AnPart q;
    q.sum[0] = sum0; q.sum[1] = sum1; q.sumsq[0] = sq0; q.sumsq[1] = sq1;
    q.segments = counted; q.skipped = skipped; q.nnon = r_n[0]; q.pad = 0;
    ppart[prow] = q;
  }
}

// The engine's reduce (kernels_welch.hpp): block (x = record of the launch, y = stream); NB3 = 3 (N / 2 + 1); the open
// records are open_*[par]: [2][S] records and [2][S][NB3] sums.  last != 0 (the call's last launch; runs may be 0): block 0
// copies the frames [max(n0, n_end - (N - 1)), n_end) of the call to the carry.
__global__ __launch_bounds__(kAnRT) void k_an_reduce(const double *__restrict__ ppsd, const AnPart *__restrict__ ppart, int runs,
                                                     int rmax, AnArgs a, int N, int L, long long M, int par,
                                                     double *__restrict__ open_psd, AnRec *__restrict__ open_rec,
                                                     double *__restrict__ ring_psd, AnRec *__restrict__ ring_rec,
                                                     const double *__restrict__ aud, long long astride,
                                                     double *__restrict__ carry, long long n_end, int last) {
  constexpr int T = kAnRT;
  const int tid = threadIdx.x, s = blockIdx.y;
  const size_t NB3 = (size_t)kAnRows * (size_t)(N / 2 + 1);
  if (runs > 0) {
    const WelchRec w = welch_rec(a, runs, rmax, L, par, gridDim.y, s, blockIdx.x);
    if (!w.done || w.keep) {
      double *dst = w.done ? ring_psd + w.slot * NB3 : open_psd + w.os_out * NB3;
      for (size_t e = tid; e < NB3; e += T) {
        double v = w.carried ? open_psd[w.os_in * NB3 + e] : 0.0;
        for (int b = 0; b < w.nsub; b++) v += ppsd[(w.p_first + b) * NB3 + e];
        dst[e] = v;
      }
      if (tid == 0) {
        AnRec o{};
        if (w.carried) o = open_rec[w.os_in];
        for (int b = 0; b < w.nsub; b++) {
          const AnPart q = ppart[w.p_first + b];
          o.sum[0] += q.sum[0]; o.sum[1] += q.sum[1]; o.sumsq[0] += q.sumsq[0]; o.sumsq[1] += q.sumsq[1];
          o.segments += q.segments; o.skipped += q.skipped; o.n_nonfinite += q.nnon;
        }
        if (w.done) {
          o.index = (uint64_t)w.l;
          o.first_sample = (uint64_t)(w.l * M);
          o.channels = (uint32_t)a.ch;
          o.fft_size = (uint32_t)N;
          o.interval_samples = (uint32_t)M;
          ring_rec[w.slot] = o;
        } else {
          open_rec[w.os_out] = o;
        }
      }
    }
  }
  if (last && blockIdx.x == 0) {
    double *row = carry + (long long)s * N * 2;
    const double *x = aud + (long long)s * astride;
    for (int q = tid; q < N - 1; q += T) {
      const long long p = n_end - (N - 1) + q;
      if (p >= a.n0) {
        const double *f = x + (p - a.n0) * a.ch;
        row[(p & (N - 1)) * 2] = f[0];
        if (a.ch == 2) row[(p & (N - 1)) * 2 + 1] = f[1];
      }
    }
  }
}

}  // namespace fmr
