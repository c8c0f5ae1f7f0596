// kernels_loudness.hpp -- audio monitor of the decoded audio (fmr_enable_loudness).
//
// Indices are absolute, counted from the chain's first audio sample.  Q = step_samples; sub-block (record) q covers the
// samples [q Q, (q + 1) Q).  A sub-block is cut into aligned chunks of C = 256 samples (the last one shorter); chunk g
// = q cps + b covers [q Q + b C, min(q Q + (b + 1) C, (q + 1) Q)), so a chunk never straddles a sub-block boundary.  A
// launch takes the samples [a0, a1) of one call: run r of the launch is chunk g0 + r clipped to them.
//
// K-weighting is a four-state linear recurrence per channel, z' = A z + B x (two biquads, ld_step).  Linear multiple
// shooting, as the DC block does it:
//   k_ld_pass1   one lane per (run, channel): the zero-state end state G of the run (4 doubles).
//   k_ld_nodes   one wave per (stream, channel): start[r + 1] = A^len(r) start[r] + G[r], from the carried state.  Every
//                map of the scan is (n, v) -> A^n z + v, so a map is its sample count and a vector; A^n v comes from
//                the table A^(2^b) (built on the host from ld_step on unit states), one product per set bit of n.
//                A lane folds its K consecutive runs, a log-step wave scan joins the lanes, the lane replays its runs.
//   k_ld_pass2   one lane per (run, channel): the run from its true start state with ld_step itself, the sum of the
//                squared K-weighted samples into a partial; the launch's last run leaves the carried state.
//   k_ld_block   one workgroup per run, one thread per sample: sum x^2, sum L R, max |x|, the true peak (12-tap, 4-phase
//                interpolator over the 11 samples behind, through LDS; before the call's first sample from the carry),
//                the non-finite count; a fixed tree over the threads.
//   k_ld_reduce  one wave per (record of the launch, stream): the record's partials in run order (lane i takes the
//                runs i, i + 64, ..., then a fixed tree), on top of the open record when the record began in an earlier
//                launch; a complete record goes to the ring [S][L], an open one to the open records (two copies by
//                launch parity).  In the call's last launch it also copies the call's last 15 samples to the carry.
//
// A non-finite sample is counted and enters everything as 0.0.  Nothing here waits on another workgroup or on the
// host, and there are no float atomics.  The translation unit is compiled with -ffp-contract=off: every product and sum
// below is rounded by itself, in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmr {

constexpr int kLdC = 256;        // chunk length in samples (= threads of k_ld_block)
constexpr int kLdHist = 16;      // slots of the true-peak carry per stream and channel: sample p at p mod 16 (reach 11)
constexpr int kLdPow = 32;       // entries of the table A^(2^b)
constexpr int kLdTaps = 12;      // true peak: taps per phase, k = -5 .. 6
constexpr int kLdMaxRuns = 1024; // runs per stream and launch at most

// fmr_loudness_record, field for field (the engine checks the sizes)
struct LdRec {
  uint64_t index, first_sample;
  uint32_t n_nonfinite, channels, step_samples, reserved;
  double kw_sumsq[2], sumsq[2], sum_lr, sample_peak[2], true_peak[2];
};

// what k_ld_block leaves per run
struct LdPart {
  double sumsq[2], sum_lr, speak[2], tpeak[2];
  unsigned nnon, pad;
};

struct LdCoef { double b0[2], b1[2], b2[2], a1[2], a2[2]; };   // stage 1, stage 2 (BS.1770-4, 48 kHz)

struct LdArgs {
  long long n0;        // absolute index of the call's first sample
  long long a0, a1;    // the launch takes the samples [a0, a1)
  long long g0;        // chunk of sample a0
  int Q, cps, ch;      // sub-block length, chunks per sub-block, channels (1 or 2: the audio is interleaved)
};

// samples [lo, hi) of chunk g (whole, before a launch clips it)
__host__ __device__ inline void ld_chunk(int Q, int cps, long long g, long long &lo, long long &hi) {
  const long long q = g / cps, b = g - q * cps;
  lo = q * Q + b * kLdC;
  hi = lo + kLdC < (q + 1) * Q ? lo + kLdC : (q + 1) * Q;
}

// one sample through both biquads: w = x - a1 w1 - a2 w2; y = b0 w + b1 w1 + b2 w2.  z = (w1, w2) of stage 1, of stage 2
__host__ __device__ inline double ld_step(const LdCoef &k, double x, double z[4]) {
  const double w = x - k.a1[0] * z[0] - k.a2[0] * z[1];
  const double y = k.b0[0] * w + k.b1[0] * z[0] + k.b2[0] * z[1];
  z[1] = z[0]; z[0] = w;
  const double v = y - k.a1[1] * z[2] - k.a2[1] * z[3];
  const double o = k.b0[1] * v + k.b1[1] * z[2] + k.b2[1] * z[3];
  z[3] = z[2]; z[2] = v;
  return o;
}

__device__ __forceinline__ double ld_clean(double v) { return isfinite(v) ? v : 0.0; }

// z <- A^n z with the table pw[b] = A^(2^b), row-major 4 x 4
__device__ __forceinline__ void ld_apow(const double *__restrict__ pw, unsigned n, double z[4]) {
  for (int b = 0; n != 0u && b < kLdPow; b++, n >>= 1) {
    if (n & 1u) {
      const double *m = pw + 16 * b;
      const double y0 = m[0] * z[0] + m[1] * z[1] + m[2] * z[2] + m[3] * z[3];
      const double y1 = m[4] * z[0] + m[5] * z[1] + m[6] * z[2] + m[7] * z[3];
      const double y2 = m[8] * z[0] + m[9] * z[1] + m[10] * z[2] + m[11] * z[3];
      const double y3 = m[12] * z[0] + m[13] * z[1] + m[14] * z[2] + m[15] * z[3];
      z[0] = y0; z[1] = y1; z[2] = y2; z[3] = y3;
    }
  }
}

// the launch's run r: its samples [lo, hi)
__device__ __forceinline__ void ld_run(const LdArgs &a, int r, long long &lo, long long &hi) {
  ld_chunk(a.Q, a.cps, a.g0 + r, lo, hi);
  lo = lo > a.a0 ? lo : a.a0;
  hi = hi < a.a1 ? hi : a.a1;
}

// a lane's serial walk over the samples [lo, hi) of channel c: eight loads in flight, then the eight dependent steps
template <class F>
__device__ __forceinline__ void ld_walk(const double *__restrict__ x, const LdArgs &a, int c, long long lo, long long hi, F &&f) {
  const double *p = x + (lo - a.n0) * a.ch + c;
  const int n = (int)(hi - lo), st = a.ch;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = p[(long long)(i + u) * st];
#pragma unroll
    for (int u = 0; u < 8; u++) f(ld_clean(v[u]));
  }
  for (; i < n; i++) f(ld_clean(p[(long long)i * st]));
}

// Lane = (run, channel) of stream blockIdx.y; the call's audio of stream s at aud + s astride (sample n0 first).
// G[((s 2 + c) rmax + run) 4 ..]: the run's end state from the zero state.
__global__ __launch_bounds__(64) void k_ld_pass1(const double *__restrict__ aud, long long astride, LdArgs a, LdCoef k,
                                                 int runs, int rmax, double *__restrict__ G) {
  const int idx = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  const int run = idx / a.ch, c = idx - run * a.ch;
  if (run >= runs) return;
  long long lo, hi;
  ld_run(a, run, lo, hi);
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  ld_walk(aud + (long long)s * astride, a, c, lo, hi, [&](double v) { (void)ld_step(k, v, z); });
  double *g = G + (((size_t)s * 2 + c) * rmax + run) * 4;
  g[0] = z[0]; g[1] = z[1]; g[2] = z[2]; g[3] = z[3];
}

// One wave per (stream, channel) = blockIdx.x: the start state of every run of the launch from the carried state
// state[(s 2 + c) 4 ..] (which k_ld_pass2 of the launch before has left).
__global__ __launch_bounds__(64) void k_ld_nodes(const double *__restrict__ G, double *__restrict__ start, LdArgs a, int runs,
                                                 int rmax, const double *__restrict__ pw, const double *__restrict__ state) {
  const int s = blockIdx.x / a.ch, c = blockIdx.x - s * a.ch, lane = threadIdx.x;
  const size_t row = ((size_t)s * 2 + c) * rmax;
  const double *g = G + row * 4;
  double *o = start + row * 4;
  const int K = (runs + 63) / 64;
  const int r0 = lane * K < runs ? lane * K : runs, r1 = r0 + K < runs ? r0 + K : runs;
  // my runs folded from the zero state: (n, q)
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  int n = 0;
  for (int r = r0; r < r1; r++) {
    long long lo, hi;
    ld_run(a, r, lo, hi);
    ld_apow(pw, (unsigned)(hi - lo), q);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] += g[(size_t)r * 4 + j];
    n += (int)(hi - lo);
  }
  // inclusive scan inside the wave: (pn, pq) then (n, q) is (pn + n, A^n pq + q)
#pragma unroll
  for (int lv = 0; lv < 6; lv++) {
    const int o_ = 1 << lv;
    double p[4];
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = __shfl_up(q[j], o_, 64);
    const int pn = __shfl_up(n, o_, 64);
    if (lane >= o_) {
      ld_apow(pw, (unsigned)n, p);
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] += p[j];
      n += pn;
    }
  }
  // my start = A^(samples before me) carry + (inclusive result of the lane before)
  double e[4];
#pragma unroll
  for (int j = 0; j < 4; j++) e[j] = __shfl_up(q[j], 1, 64);
  int en = __shfl_up(n, 1, 64);
  if (lane == 0) { e[0] = e[1] = e[2] = e[3] = 0.0; en = 0; }
  double x[4];
#pragma unroll
  for (int j = 0; j < 4; j++) x[j] = state[((size_t)s * 2 + c) * 4 + j];
  ld_apow(pw, (unsigned)en, x);
#pragma unroll
  for (int j = 0; j < 4; j++) x[j] += e[j];
  for (int r = r0; r < r1; r++) {
#pragma unroll
    for (int j = 0; j < 4; j++) o[(size_t)r * 4 + j] = x[j];
    long long lo, hi;
    ld_run(a, r, lo, hi);
    ld_apow(pw, (unsigned)(hi - lo), x);
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] += g[(size_t)r * 4 + j];
  }
}

// Lane = (run, channel) as in pass 1: the run from its start state; pkw[(s 2 + c) rmax + run] = sum of the squared
// K-weighted samples, in sample order.  The launch's last run leaves the state for the next launch.
__global__ __launch_bounds__(64) void k_ld_pass2(const double *__restrict__ aud, long long astride, LdArgs a, LdCoef k,
                                                 int runs, int rmax, const double *__restrict__ start,
                                                 double *__restrict__ pkw, double *__restrict__ state) {
  const int idx = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  const int run = idx / a.ch, c = idx - run * a.ch;
  if (run >= runs) return;
  long long lo, hi;
  ld_run(a, run, lo, hi);
  const size_t row = ((size_t)s * 2 + c) * rmax + run;
  double z[4] = {start[row * 4], start[row * 4 + 1], start[row * 4 + 2], start[row * 4 + 3]};
  double acc = 0.0;
  ld_walk(aud + (long long)s * astride, a, c, lo, hi, [&](double v) {
    const double y = ld_step(k, v, z);
    acc += y * y;
  });
  pkw[row] = acc;
  if (run == runs - 1) {
    double *st = state + ((size_t)s * 2 + c) * 4;
    st[0] = z[0]; st[1] = z[1]; st[2] = z[2]; st[3] = z[3];
  }
}

// Workgroup = (run, stream), thread t = sample lo + t of the run.  taps[p - 1][k + 5] = g_p[k], p = 1 .. 3 (p = 0 is the
// identity: x[n - 6] itself).  hist[(s 2 + c) 16 + (p mod 16)]: the samples before the call's first one.
__global__ __launch_bounds__(kLdC) void k_ld_block(const double *__restrict__ aud, long long astride, LdArgs a, int rmax,
                                                   const double *__restrict__ taps, const double *__restrict__ hist,
                                                   LdPart *__restrict__ part) {
  constexpr int T = kLdC, R = kLdTaps - 1;
  __shared__ double xs[2][T + R];
  __shared__ double r_a[T], r_b[T];
  __shared__ unsigned r_n[T];
  const int tid = threadIdx.x, run = blockIdx.x, s = blockIdx.y;
  long long lo, hi;
  ld_run(a, run, lo, hi);
  const int len = (int)(hi - lo);
  const double *x = aud + (long long)s * astride;
  unsigned nnon = 0;
  // the samples [lo - 11, hi) of both channels, cleaned, at xs[c][p - lo + 11]
  for (int c = 0; c < a.ch; c++) {
    for (int i = tid; i < len + R; i += T) {
      const long long p = lo - R + i;
      double v = 0.0;
      if (p >= a.n0) v = x[(p - a.n0) * a.ch + c];
      else if (p >= 0) v = hist[((size_t)s * 2 + c) * kLdHist + (p & (kLdHist - 1))];
      if (i >= R && !isfinite(v)) nnon++;
      xs[c][i] = ld_clean(v);
    }
  }
  __syncthreads();
  double sq[2] = {0.0, 0.0}, sp[2] = {0.0, 0.0}, tp[2] = {0.0, 0.0}, lr = 0.0;
  if (tid < len) {
    for (int c = 0; c < a.ch; c++) {
      const double *w = &xs[c][tid];            // w[j] = x[n - 11 + j]: the sum's x[n - 6 + k] is w[k + 5]
      const double v = w[R];
      sq[c] = v * v;
      sp[c] = fabs(v);
      double m = fabs(w[5]);
#pragma unroll
      for (int p = 0; p < 3; p++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kLdTaps; j++) acc += w[j] * taps[p * kLdTaps + j];
        m = fmax(m, fabs(acc));
      }
      tp[c] = m;
    }
    if (a.ch == 2) lr = xs[0][tid + R] * xs[1][tid + R];
  }
  // a fixed tree over the threads, two values at a time
  auto tree = [&](double &u, double &v, bool is_max) {
    __syncthreads();
    r_a[tid] = u; r_b[tid] = v;
    __syncthreads();
    for (int st = T / 2; st > 0; st >>= 1) {
      if (tid < st) {
        r_a[tid] = is_max ? fmax(r_a[tid], r_a[tid + st]) : r_a[tid] + r_a[tid + st];
        r_b[tid] = is_max ? fmax(r_b[tid], r_b[tid + st]) : r_b[tid] + r_b[tid + st];
      }
      __syncthreads();
    }
    u = r_a[0]; v = r_b[0];
  };
  tree(sq[0], sq[1], false);
  tree(sp[0], sp[1], true);
  tree(tp[0], tp[1], true);
  double dummy = 0.0;
  tree(lr, dummy, false);
  __syncthreads();
  r_n[tid] = nnon;
  __syncthreads();
  for (int st = T / 2; st > 0; st >>= 1) {
    if (tid < st) r_n[tid] += r_n[tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    LdPart q;
    q.sumsq[0] = sq[0]; q.sumsq[1] = sq[1]; q.sum_lr = lr;
    q.speak[0] = sp[0]; q.speak[1] = sp[1]; q.tpeak[0] = tp[0]; q.tpeak[1] = tp[1];
    q.nnon = r_n[0]; q.pad = 0;
    part[(size_t)s * rmax + run] = q;
  }
}

__device__ __forceinline__ double ld_wave_sum(double v) {      // lane 0 holds the sum, a fixed tree
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ double ld_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}

// Wave (x = record l0 + blockIdx.x of the launch, y = stream); l0 = the record of sample a0.  open_rec: [2][S], ring:
// [S][L].  A complete record goes to slot (index mod L) unless a later record of the same launch takes that slot; an
// open one to open_rec[par ^ 1]: the wave that reads the old copy is not the one that writes the new one.  last != 0
// (the call's last launch): wave 0 copies the samples [max(n0, a1 - 15), a1) of the call to the carry.
__global__ __launch_bounds__(64) void k_ld_reduce(const double *__restrict__ pkw, const LdPart *__restrict__ part, int runs,
                                                  int rmax, LdArgs a, int L, int par, LdRec *__restrict__ open_rec,
                                                  LdRec *__restrict__ ring, const double *__restrict__ aud,
                                                  long long astride, double *__restrict__ hist, int last) {
  const int lane = threadIdx.x, s = blockIdx.y, S = gridDim.y;
  const long long l = a.a0 / a.Q + blockIdx.x;
  const long long g_last = a.g0 + runs - 1;
  const int b_lo = blockIdx.x == 0 ? (int)(a.g0 - l * a.cps) : 0;
  const int b_hi = (int)(a.cps < g_last - l * a.cps + 1 ? a.cps : g_last - l * a.cps + 1);
  double kw[2] = {0.0, 0.0}, sq[2] = {0.0, 0.0}, sp[2] = {0.0, 0.0}, tp[2] = {0.0, 0.0}, lr = 0.0;
  unsigned nnon = 0;
  for (int b = b_lo + lane; b < b_hi; b += 64) {
    const size_t r = (size_t)(l * a.cps + b - a.g0);
    const LdPart q = part[(size_t)s * rmax + r];
#pragma unroll
    for (int c = 0; c < 2; c++) {
      if (c < a.ch) kw[c] += pkw[((size_t)s * 2 + c) * rmax + r];
      sq[c] += q.sumsq[c];
      sp[c] = fmax(sp[c], q.speak[c]);
      tp[c] = fmax(tp[c], q.tpeak[c]);
    }
    lr += q.sum_lr;
    nnon += q.nnon;
  }
#pragma unroll
  for (int c = 0; c < 2; c++) {
    kw[c] = ld_wave_sum(kw[c]); sq[c] = ld_wave_sum(sq[c]);
    sp[c] = ld_wave_max(sp[c]); tp[c] = ld_wave_max(tp[c]);
  }
  lr = ld_wave_sum(lr);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nnon += __shfl_down(nnon, o, 64);
  if (lane == 0) {
    LdRec o{};
    if (a.a0 > l * a.Q) o = open_rec[(size_t)par * S + s];      // the record began in an earlier launch
#pragma unroll
    for (int c = 0; c < 2; c++) {
      o.kw_sumsq[c] += kw[c]; o.sumsq[c] += sq[c];
      o.sample_peak[c] = fmax(o.sample_peak[c], sp[c]);
      o.true_peak[c] = fmax(o.true_peak[c], tp[c]);
    }
    o.sum_lr += lr;
    o.n_nonfinite += nnon;
    const long long last_done = a.a1 / a.Q - 1;                 // last record complete after this launch
    if (l <= last_done) {
      if (l + L > last_done) {
        o.index = (uint64_t)l;
        o.first_sample = (uint64_t)(l * a.Q);
        o.channels = (uint32_t)a.ch;
        o.step_samples = (uint32_t)a.Q;
        ring[(size_t)s * L + (size_t)(l % L)] = o;
      }
    } else {
      open_rec[(size_t)(par ^ 1) * S + s] = o;
    }
  }
  if (last && blockIdx.x == 0 && lane < (kLdHist - 1) * a.ch) {
    const int c = lane % a.ch;
    const long long p = a.a1 - (kLdHist - 1) + lane / a.ch;
    if (p >= a.n0)
      hist[((size_t)s * 2 + c) * kLdHist + (p & (kLdHist - 1))] = aud[(long long)s * astride + (p - a.n0) * a.ch + c];
  }
}

}  // namespace fmr
