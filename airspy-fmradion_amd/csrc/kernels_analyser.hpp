// kernels_analyser.hpp -- audio analyser of the decoded audio (fmr_enable_analyser).
//
// Indices are absolute, counted from the chain's first audio sample (a frame: one sample per channel).  N = fft_size
// (1024 .. 8192), H = N / 2, M = interval_samples (a multiple of H).  Record i covers the frames [i M, (i + 1) M);
// segment j covers [j H, j H + N) and belongs to record floor(j H / M) (the rule of kernels_monitor.hpp): a record holds
// M / H segments, and its last one reaches H frames into the next record.  A segment is processed in the call that
// delivers its last frame; the time-domain part of a record (sum, sum of squares, non-finite count) is taken over the
// FIRST H frames of each of its segments, so every frame enters it exactly once wherever a call ends.
//
// k_an_seg<LOGN>: one workgroup = one run of segments of one stream.  A record is cut into aligned sub-blocks of `sub`
// segments (fixed per chain; the last one shorter); run r of a launch is sub-block g0 + r clipped to the launch's
// segments, so a run never straddles a record boundary.  Per segment: N frames of fp64 audio from the call (or, in front
// of the call's first frame, from the stream's carry of the last N frames, frame p at p mod N), each sample rounded once
// to fp32 and multiplied by the fp32 window, z[n] = wL[n] + i wR[n] stored bit-reversed into padded LDS, then the radix-2
// pass (odd log2 N) and the radix-4 decimation-in-time passes in place.  With X = Z[k] and Y = conj Z[(N - k) mod N]:
// L[k] = (X + Y) / 2, R[k] = (X - Y) / (2 i) in fp32; |L|^2, |R|^2 and Re(L conj R) are formed in fp64 from those fp32
// values and folded into fp64 registers across the run, k = 0 .. N / 2.  With one channel the imaginary input is 0, the
// first row is |Z[k]|^2 and the other two stay 0.  A segment that holds a sample which is not finite as fp32 is skipped
// for the spectral part and counted; the time-domain part takes its finite samples as they are and the others as 0.
// One partial per run.
//
// k_an_reduce: one workgroup per (stream, record the launch touches) adds the record's partials in run order (fp64, no
// float atomics) on top of the stream's open record when the record began in an earlier launch; a complete record goes to
// slot index mod L of the ring [S][L], an open one to the other copy of the open record (two copies by launch parity).  In
// the call's last launch it also copies the call's last N - 1 frames into the carry.
//
// Nothing here waits on another workgroup or on the host.  The scaling to power, c_k / (N sum w^2 segments), happens on the
// host when a record is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"               // (kernels_spectrum.hpp needs fmr::IqFmt)
#include "kernels_spectrum.hpp"      // spec_pad, cmul

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

struct AnArgs {
  long long n0;        // absolute index of the call's first frame
  long long a0, a1;    // the launch takes the segments [a0, a1)
  long long g0;        // sub-block of segment a0
  int spr, sub, sb;    // segments per record, per sub-block, sub-blocks per record = ceil(spr / sub)
  int ch;              // channels (1 or 2: the audio is interleaved)
};

// segments [lo, hi) of sub-block g (whole, before a launch clips it)
__host__ __device__ inline void an_sub(int spr, int sub, int sb, long long g, long long &lo, long long &hi) {
  const long long l = g / sb, b = g - l * sb;
  lo = l * spr + b * sub;
  hi = lo + sub < (l + 1) * spr ? lo + sub : (l + 1) * spr;
}

// The N-point FFT over the bit-reversed points in lds: one radix-2 pass when log2 N is odd, then radix-4 decimation-in-
// time passes in place; every thread owns whole butterflies, one barrier per pass, the output in natural order.
template <int LOGN>
__device__ __forceinline__ void an_fft(float2 *lds, const float2 *__restrict__ tw, int tid) {
  using S = AnShape<LOGN>;
  constexpr int N = S::N, T = S::T;
  int span = 1;
  if (LOGN & 1) {
#pragma unroll
    for (int q = 0; q < N / 2 / T; q++) {
      const int b = tid + q * T;
      const int e0 = spec_pad(2 * b), e1 = spec_pad(2 * b + 1);
      const float2 a0 = lds[e0], a1 = lds[e1];
      lds[e0] = make_float2(a0.x + a1.x, a0.y + a1.y);
      lds[e1] = make_float2(a0.x - a1.x, a0.y - a1.y);
    }
    span = 2;
    __syncthreads();
  }
  // four length-span sub-DFTs at block offsets 0, span, 2 span, 3 span (bit-reversed: the residues 0, 2, 1, 3 of the
  // length-4 span DFT) -> one length-4 span DFT; W_{4 span}^{j k} = tw[j k N / (4 span)]
  for (; span < N; span *= 4) {
    const int tstep = N / (4 * span);
#pragma unroll 1
    for (int q = 0; q < N / 4 / T; q++) {
      const int b = tid + q * T;
      const int jj = b & (span - 1);
      const int base = (b - jj) * 4 + jj;
      const int e0 = spec_pad(base), e1 = spec_pad(base + span), e2 = spec_pad(base + 2 * span), e3 = spec_pad(base + 3 * span);
      const float2 a0 = lds[e0];
      const float2 a1 = cmul(lds[e2], tw[jj * tstep]);
      const float2 a2 = cmul(lds[e1], tw[2 * jj * tstep]);
      const float2 a3 = cmul(lds[e3], tw[3 * jj * tstep]);
      const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
      const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
      // X0 = s02 + s13, X1 = d02 - i d13, X2 = s02 - s13, X3 = d02 + i d13
      lds[e0] = make_float2(s02.x + s13.x, s02.y + s13.y);
      lds[e1] = make_float2(d02.x + d13.y, d02.y - d13.x);
      lds[e2] = make_float2(s02.x - s13.x, s02.y - s13.y);
      lds[e3] = make_float2(d02.x - d13.y, d02.y + d13.x);
    }
    __syncthreads();
  }
}

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
  an_sub(a.spr, a.sub, a.sb, a.g0 + run, lo, hi);
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
    an_fft<LOGN>(lds_an, tw, tid);
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

// Block (x = record l0 + blockIdx.x of the launch, y = stream); l0 = the record of segment a0; NB3 = 3 (N / 2 + 1).  The
// block adds the partials of its record's sub-blocks inside the launch in run order, starting from the open record of
// the launch before (open_*[par]: [2][S] records and [2][S][NB3] sums) when the record began there.  A record whose last
// segment is in goes to slot (index mod L) of the rings -- unless a later record of the same launch takes that slot --, an
// open one to open_*[par ^ 1]: the block that reads the old copy is not the one that writes the new one.  last != 0 (the
// call's last launch; runs may be 0): block 0 copies the frames [max(n0, n_end - (N - 1)), n_end) of the call to the carry.
__global__ __launch_bounds__(kAnRT) void k_an_reduce(const double *__restrict__ ppsd, const AnPart *__restrict__ ppart, int runs,
                                                     int rmax, AnArgs a, int N, int L, long long M, int par,
                                                     double *__restrict__ open_psd, AnRec *__restrict__ open_rec,
                                                     double *__restrict__ ring_psd, AnRec *__restrict__ ring_rec,
                                                     const double *__restrict__ aud, long long astride,
                                                     double *__restrict__ carry, long long n_end, int last) {
  constexpr int T = kAnRT;
  const int tid = threadIdx.x, s = blockIdx.y, S = gridDim.y;
  const size_t NB3 = (size_t)kAnRows * (size_t)(N / 2 + 1);
  if (runs > 0) {
    const long long l = a.g0 / a.sb + blockIdx.x;
    const long long g_last = a.g0 + runs - 1;
    const int b_lo = blockIdx.x == 0 ? (int)(a.g0 - l * a.sb) : 0;
    const int b_hi = (int)(a.sb < g_last - l * a.sb + 1 ? a.sb : g_last - l * a.sb + 1);
    const bool carried = a.a0 > l * a.spr;          // the record began in an earlier launch (the launch's first record only)
    const long long last_done = a.a1 / a.spr - 1;   // last record complete after this launch
    const bool done = l <= last_done, keep = l + L > last_done;
    const size_t os_in = ((size_t)par * S + s), os_out = ((size_t)(par ^ 1) * S + s);
    const size_t slot = (size_t)s * L + (size_t)(l % L);
    const size_t p_first = (size_t)s * rmax + (size_t)(l * a.sb + b_lo - a.g0);
    if (!done || keep) {
      double *dst = done ? ring_psd + slot * NB3 : open_psd + os_out * NB3;
      for (size_t e = tid; e < NB3; e += T) {
        double v = carried ? open_psd[os_in * NB3 + e] : 0.0;
        for (int b = 0; b < b_hi - b_lo; b++) v += ppsd[(p_first + b) * NB3 + e];
        dst[e] = v;
      }
      if (tid == 0) {
        AnRec o{};
        if (carried) o = open_rec[os_in];
        for (int b = 0; b < b_hi - b_lo; b++) {
          const AnPart q = ppart[p_first + b];
          o.sum[0] += q.sum[0]; o.sum[1] += q.sum[1]; o.sumsq[0] += q.sumsq[0]; o.sumsq[1] += q.sumsq[1];
          o.segments += q.segments; o.skipped += q.skipped; o.n_nonfinite += q.nnon;
        }
        if (done) {
          o.index = (uint64_t)l;
          o.first_sample = (uint64_t)(l * M);
          o.channels = (uint32_t)a.ch;
          o.fft_size = (uint32_t)N;
          o.interval_samples = (uint32_t)M;
          ring_rec[slot] = o;
        } else {
          open_rec[os_out] = o;
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
