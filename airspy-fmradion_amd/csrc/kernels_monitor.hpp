// kernels_monitor.hpp -- modulation monitor of the 384 kHz MPX (fmr_enable_monitor).
//
// An instance of the Welch segment engine (kernels_welch.hpp: indices, the partition into sub-blocks and runs, the carry,
// the open records and the ring) with N = 1024, H = 512, M = interval_samples and sub-blocks of 4 .. 32 segments.  What
// is this stage's own:
//
// k_mon_seg: one workgroup (256 threads) = one run.  Per segment: 1024 floats from the call's MPX or the carry, the
// time-domain part of a record (counts, min, max, sum, sum of squares, histogram through LDS integer atomics) over the
// segment's FIRST 512 samples -- so every sample enters it exactly once, in the segment it starts, wherever a call ends --,
// then window, bit-reversed store, welch_fft and |X[k]|^2 of the bins 0 .. 512 into fp64 registers.  A segment with a
// non-finite sample is skipped for the spectral part and counted; its finite samples still enter the time-domain part.
// The run's values go to a partial once.
//
// k_mon_reduce: the engine's reduce over PSD sums, histogram counters and MonRec; in the call's last launch it also
// copies the call's last 1023 samples into the carry.
//
// The bodies of both kernels (mon_seg_run, mon_reduce_run) are shared with the RF monitor (kernels_rfmon.hpp), which
// differs in where a sample comes from and in the histogram's bin rule.
//
// The density scaling c_k / (F sum w^2) and the division by the segment count happen on the host when a record is read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_welch.hpp"

namespace fmr {

constexpr int kMonLog = 10, kMonN = 1 << kMonLog, kMonH = kMonN / 2, kMonPsd = kMonN / 2 + 1;
constexpr int kMonT = 256;             // threads of both kernels: one radix-4 butterfly each per pass
constexpr int kMonSubMin = 4, kMonSubMax = 32;   // segments per sub-block of a record (per chain: MonArgs::sub)
constexpr int kMonMaxHist = 1024;

// fmr_monitor_record, field for field (the engine checks the sizes); mn / mx hold +inf / -inf while nothing finite is in
struct MonRec {
  uint64_t index, first_sample;
  uint32_t n_finite, n_nonfinite, segments, skipped;
  float mn, mx;
  double sum, sumsq;
};

struct MonArgs : WelchArgs {
  int bins;            // histogram: B, Rf = (float)R, scale = (float)(B / (2 R))
  float rf, scale;
};

// the histogram's bin rule, unfused fp32 (the clamp runs on the float: a huge sample never reaches the conversion)
__device__ __forceinline__ int mon_bin(float x, float rf, float scale, int bins) {
  float t = floorf((x + rf) * scale);
  t = t < 0.f ? 0.f : t;
  t = t > (float)(bins - 1) ? (float)(bins - 1) : t;
  return (int)t;
}

// Where a segment kernel's samples come from and how they are binned: the MPX of the modulation monitor here, the IF
// power of the RF monitor in kernels_rfmon.hpp.  at(p) is the sample of absolute index p (from the call, or in front of
// its first sample from the stream's carry), bin(v) the histogram counter of a finite sample, fresh(i) sample i of the
// call (what the carry keeps); make() builds stream s's source from the kernels' arguments (cin = that stream's carry).
struct MonMpxSrc {
  static constexpr int kHist = kMonMaxHist;
  const float *xin, *cin;
  long long n0;
  float rf, scale;
  int bins;
  __device__ __forceinline__ static MonMpxSrc make(const void *base, long long stride, int off, int s, const float *cin,
                                                   const MonArgs &a) {
    return {reinterpret_cast<const float *>(base) + (long long)s * stride + off, cin, a.n0, a.rf, a.scale, a.bins};
  }
  __device__ __forceinline__ float fresh(long long i) const { return xin[i]; }
  __device__ __forceinline__ float at(long long p) const { return p < n0 ? cin[p & (kMonN - 1)] : xin[p - n0]; }
  __device__ __forceinline__ int bin(float v) const { return mon_bin(v, rf, scale, bins); }
};

// One run of segments of stream s (the body of both monitors' segment kernels): run `run` of the launch, samples from
// src.  Partials of the run at row s rmax + run: ppsd [kMonPsd], phist [a.bins], prec.
template <class Src>
__device__ __forceinline__ void mon_seg_run(const Src &src, int run, int s, const MonArgs &a, const float *__restrict__ win,
                                            const float2 *__restrict__ tw, int rmax, double *__restrict__ ppsd,
                                            unsigned *__restrict__ phist, MonRec *__restrict__ prec) {
  constexpr int N = kMonN, T = kMonT;
  __shared__ float2 lds[N + (N >> 5)];
  __shared__ unsigned s_hist[Src::kHist];
  const int tid = threadIdx.x;
  long long lo, hi;
  welch_sub(a.spr, a.sub, a.sb, a.g0 + run, lo, hi);
  const long long j_lo = lo > a.a0 ? lo : a.a0, j_hi = hi < a.a1 ? hi : a.a1;
  for (int b = tid; b < a.bins; b += T) s_hist[b] = 0u;
  __syncthreads();

  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;       // bins tid, tid + 256 and (thread 0) 512
  double sum = 0.0, sumsq = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  unsigned nfin = 0, nnon = 0, counted = 0, skipped = 0;

  for (long long j = j_lo; j < j_hi; j++) {
    const long long p0 = j * kMonH;
    int bad = 0;
#pragma unroll
    for (int q = 0; q < N / T; q++) {
      const int i = tid + q * T;
      const long long p = p0 + i;
      const float v = src.at(p);
      const bool fin = isfinite(v);
      bad |= !fin;
      if (q < kMonH / T) {                 // the segment's first H samples: the time-domain part
        if (fin) {
          nfin++;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          sum += (double)v;
          sumsq += (double)v * (double)v;
          atomicAdd(&s_hist[src.bin(v)], 1u);
        } else {
          nnon++;
        }
      }
      lds[spec_pad((int)(__brev((unsigned)i) >> (32 - kMonLog)))] = make_float2(v * win[i], 0.f);
    }
    bad = __syncthreads_or(bad);
    if (bad) { skipped++; continue; }      // (uniform: nobody has read the LDS, the next segment's stores may follow)
    welch_fft<kMonLog, kMonT>(lds, tw, tid);
    {
      const float2 x0 = lds[spec_pad(tid)], x1 = lds[spec_pad(tid + T)];
      acc0 += (double)(x0.x * x0.x + x0.y * x0.y);
      acc1 += (double)(x1.x * x1.x + x1.y * x1.y);
      if (tid == 0) {
        const float2 x2 = lds[spec_pad(N / 2)];
        acc2 += (double)(x2.x * x2.x + x2.y * x2.y);
      }
    }
    counted++;
    __syncthreads();                       // every thread has read its bins before the next segment's stores
  }

  // the run's time-domain values: a fixed tree over the 256 threads (the FFT's LDS is free now)
  __syncthreads();
  double *r_sum = reinterpret_cast<double *>(lds), *r_sq = r_sum + T;
  float *r_mn = reinterpret_cast<float *>(r_sq + T), *r_mx = r_mn + T;
  unsigned *r_fin = reinterpret_cast<unsigned *>(r_mx + T), *r_non = r_fin + T;      // 8 KiB of the 8448 bytes
  r_sum[tid] = sum; r_sq[tid] = sumsq; r_mn[tid] = mn; r_mx[tid] = mx; r_fin[tid] = nfin; r_non[tid] = nnon;
  __syncthreads();
  for (int st = T / 2; st > 0; st >>= 1) {
    if (tid < st) {
      r_sum[tid] += r_sum[tid + st];
      r_sq[tid] += r_sq[tid + st];
      r_mn[tid] = fminf(r_mn[tid], r_mn[tid + st]);
      r_mx[tid] = fmaxf(r_mx[tid], r_mx[tid + st]);
      r_fin[tid] += r_fin[tid + st];
      r_non[tid] += r_non[tid + st];
    }
    __syncthreads();
  }
  const size_t prow = (size_t)s * rmax + run;
  ppsd[prow * kMonPsd + tid] = acc0;
  ppsd[prow * kMonPsd + tid + T] = acc1;
  for (int b = tid; b < a.bins; b += T) phist[prow * a.bins + b] = s_hist[b];
  if (tid == 0) {
    ppsd[prow * kMonPsd + N / 2] = acc2;
    MonRec r;
    r.index = 0; r.first_sample = 0;
    r.n_finite = r_fin[0]; r.n_nonfinite = r_non[0]; r.segments = counted; r.skipped = skipped;
    r.mn = r_mn[0]; r.mx = r_mx[0]; r.sum = r_sum[0]; r.sumsq = r_sq[0];
    prec[prow] = r;
  }
}

// Both monitors' segment kernel, Src = MonMpxSrc | RfmSrc<NRM>.  Stream s = blockIdx.y: the call's samples as
// Src::make reads them (the MPX at (float *)from + s stride + off, sample n0 first; the IF ring slot in kernels_rfmon.hpp),
// the carry at carry + s kMonN.  Partials of run r = blockIdx.x at row s rmax + r.
template <class Src>
__global__ __launch_bounds__(kMonT) void k_mon_seg(const void *__restrict__ from, long long stride, int off,
                                                   const float *__restrict__ carry, MonArgs a,
                                                   const float *__restrict__ win, const float2 *__restrict__ tw, int rmax,
                                                   double *__restrict__ ppsd, unsigned *__restrict__ phist,
                                                   MonRec *__restrict__ prec) {
  const int s = blockIdx.y;
  const Src src = Src::make(from, stride, off, s, carry + (long long)s * kMonN, a);
  mon_seg_run(src, blockIdx.x, s, a, win, tw, rmax, ppsd, phist, prec);
}

// The record part of both monitors' reduce kernels (runs > 0): block (x = record l0 + blockIdx.x of the launch,
// y = stream), HB = counters per thread (the histogram holds at most HB kMonT of them).
template <int HB>
__device__ __forceinline__ void mon_reduce_run(const double *__restrict__ ppsd, const unsigned *__restrict__ phist,
                                               const MonRec *__restrict__ prec, int runs, int rmax, const MonArgs &a, int L,
                                               long long M, int par, double *__restrict__ open_psd,
                                               unsigned *__restrict__ open_hist, MonRec *__restrict__ open_rec,
                                               double *__restrict__ ring_psd, unsigned *__restrict__ ring_hist,
                                               MonRec *__restrict__ ring_rec) {
  constexpr int T = kMonT;
  const int tid = threadIdx.x;
  const WelchRec w = welch_rec(a, runs, rmax, L, par, gridDim.y, blockIdx.y, blockIdx.x);
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  unsigned h[HB];
#pragma unroll
  for (int k = 0; k < HB; k++) h[k] = 0u;
  MonRec o{};
  o.mn = INFINITY; o.mx = -INFINITY;
  if (w.carried) {
    const size_t os = w.os_in;
    p0 = open_psd[os * kMonPsd + tid];
    p1 = open_psd[os * kMonPsd + tid + T];
#pragma unroll
    for (int k = 0; k < HB; k++)
      if (tid + k * T < a.bins) h[k] = open_hist[os * a.bins + tid + k * T];
    if (tid == 0) { p2 = open_psd[os * kMonPsd + kMonN / 2]; o = open_rec[os]; }
  }
  for (int b = 0; b < w.nsub; b++) {
    const size_t prow = w.p_first + b;
    p0 += ppsd[prow * kMonPsd + tid];
    p1 += ppsd[prow * kMonPsd + tid + T];
#pragma unroll
    for (int k = 0; k < HB; k++)
      if (tid + k * T < a.bins) h[k] += phist[prow * a.bins + tid + k * T];
    if (tid == 0) {
      const MonRec q = prec[prow];
      p2 += ppsd[prow * kMonPsd + kMonN / 2];
      o.n_finite += q.n_finite; o.n_nonfinite += q.n_nonfinite; o.segments += q.segments; o.skipped += q.skipped;
      o.mn = fminf(o.mn, q.mn); o.mx = fmaxf(o.mx, q.mx);
      o.sum += q.sum; o.sumsq += q.sumsq;
    }
  }
  if (w.done) {
    if (w.keep) {
      const size_t slot = w.slot;
      ring_psd[slot * kMonPsd + tid] = p0;
      ring_psd[slot * kMonPsd + tid + T] = p1;
#pragma unroll
      for (int k = 0; k < HB; k++)
        if (tid + k * T < a.bins) ring_hist[slot * a.bins + tid + k * T] = h[k];
      if (tid == 0) {
        ring_psd[slot * kMonPsd + kMonN / 2] = p2;
        o.index = (uint64_t)w.l;
        o.first_sample = (uint64_t)(w.l * M);
        if (o.n_finite == 0) { o.mn = 0.f; o.mx = 0.f; }
        ring_rec[slot] = o;
      }
    }
  } else {
    const size_t os = w.os_out;
    open_psd[os * kMonPsd + tid] = p0;
    open_psd[os * kMonPsd + tid + T] = p1;
#pragma unroll
    for (int k = 0; k < HB; k++)
      if (tid + k * T < a.bins) open_hist[os * a.bins + tid + k * T] = h[k];
    if (tid == 0) { open_psd[os * kMonPsd + kMonN / 2] = p2; open_rec[os] = o; }
  }
}

// The engine's reduce (kernels_welch.hpp): block (x = record of the launch, y = stream); the open records are open_*[par]:
// [2][S] records, [2][S][bins] counters, [2][S][kMonPsd] sums.  last != 0 (the call's last launch; runs may be 0): block 0
// copies the samples [max(n0, n_end - 1023), n_end) of the call, as Src::fresh gives them, to the carry.
// Src = MonMpxSrc | RfmSrc<NRM>.
template <class Src>
__global__ __launch_bounds__(kMonT) void k_mon_reduce(const double *__restrict__ ppsd, const unsigned *__restrict__ phist,
                                                      const MonRec *__restrict__ prec, int runs, int rmax, MonArgs a,
                                                      int L, long long M, int par, double *__restrict__ open_psd,
                                                      unsigned *__restrict__ open_hist, MonRec *__restrict__ open_rec,
                                                      double *__restrict__ ring_psd, unsigned *__restrict__ ring_hist,
                                                      MonRec *__restrict__ ring_rec, const void *__restrict__ from,
                                                      long long stride, int off, float *__restrict__ carry,
                                                      long long n_end, int last) {
  constexpr int T = kMonT;
  const int tid = threadIdx.x, s = blockIdx.y;
  if (runs > 0)
    mon_reduce_run<(Src::kHist + T - 1) / T>(ppsd, phist, prec, runs, rmax, a, L, M, par, open_psd, open_hist, open_rec,
                                             ring_psd, ring_hist, ring_rec);
  if (last && blockIdx.x == 0) {
    float *row = carry + (long long)s * kMonN;
    const Src src = Src::make(from, stride, off, s, row, a);
    for (int q = tid; q < kMonN - 1; q += T) {
      const long long p = n_end - (kMonN - 1) + q;
      if (p >= a.n0) row[p & (kMonN - 1)] = src.fresh(p - a.n0);
    }
  }
}

}  // namespace fmr
