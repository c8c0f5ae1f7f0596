// kernels_weaksignal.hpp -- weak-signal handling of an FM chain (fmr_enable_weak_signal): the
// ultrasonic-noise detector on the 384 kHz MPX, the attack / release control, and stereo blend, high cut and soft mute on
// the finished audio.
//
// Indices are absolute: MPX samples from the chain's first MPX sample, audio frames from its first audio frame.  A control
// interval is Q = 768 MPX samples, interval j = [j Q, (j + 1) Q); an audio interval is A = 96 frames.  A call hands in the
// MPX samples [n0, n1) and the audio frames [f0, f1).
//
//   k_ws_usn      one workgroup per (interval the call touches, stream): the piece of the interval inside [n0, n1) and
//                 the 62 samples in front of it through LDS (in front of n0 from the stream's carry of 64 samples, sample
//                 p at p mod 64), the 63-tap fp64 FIR with k ascending, y^2, a fixed tree over the 256 threads: one
//                 partial (sum, non-finite count) per piece.
//   k_ws_control  one wave per stream: 64 intervals per load; the piece on top of the carried open partial, u = sum / Q;
//                 the recurrence s' = s + c (u - s) in order on lane broadcasts; 10 log10 and the three clamps per lane;
//                 the t values into the control ring (interval j at j mod ring length); then the records in interval
//                 order on lane broadcasts, a complete one to ring slot (index mod L).  The same wave reads and writes the
//                 stream's state (s, the open partial, the open record), so it is kept in place.  It also copies the
//                 call's last 63 samples to the carry.
//   k_ws_pass1    lane = (chunk, stream), a chunk being audio interval g clipped to [f0, f1): the zero-state end of the
//                 one-pole w of both channels, its input x1 computed on the fly from L, R and the ramped t_blend.
//   k_ws_nodes    one wave per (stream, channel): start[r + 1] = beta^len(r) start[r] + G[r] from the carried w; a map is
//                 (n, v) standing for w -> beta^n w + v, beta^n from the table beta^(2^b).
//   k_ws_pass2    lane = (chunk, stream): x1 again, w from its start state, the crossfade, the gain, the frame stored in
//                 place (a lane reads and writes only its own chunk, both channels); the last chunk leaves the carry.
//
// A non-finite MPX sample is counted in its interval and enters the FIR as 0.  Nothing here waits on another workgroup
// or on the host, and there are no float atomics.  The translation unit is compiled with -ffp-contract=off: every product
// and sum below is rounded by itself, in the order written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmr {

constexpr int kWsQ = 768;        // MPX samples per control interval (2 ms)
constexpr int kWsA = 96;         // audio frames per audio interval (= chunk length)
constexpr int kWsTaps = 63;      // detector taps
constexpr int kWsHist = 64;      // slots of the MPX carry per stream (reach 62)
constexpr int kWsT = 256;        // threads of k_ws_usn: three samples each
constexpr int kWsPow = 32;       // entries of the table beta^(2^b)

// fmr_weak_signal_record, field for field (the stage checks the size)
struct WsRec {
  uint64_t index, first_interval;
  uint32_t n_intervals, n_nonfinite;
  double usn_sum, usn_peak, smoothed, t_blend, t_highcut, t_mute, max_blend, max_highcut, max_mute;
};

struct WsPart { double sumsq; unsigned nnon, pad; };      // what k_ws_usn leaves per piece
struct WsCtl { double t[3]; };                            // blend, high cut, mute of one interval

struct WsCoef {
  double c_att, c_rel;         // 1 - exp(-2 / tau_ms)
  double lo[3], hi[3];         // per action, in dB
  int on[3];
  int R, L;                    // intervals per record, records per ring
};

// what a stream carries from call to call
struct WsState {
  double s;                    // s of the last complete interval
  double open_sum;             // the open interval: sum of y^2 so far, non-finite samples so far
  unsigned open_non, pad;
  WsRec open;                  // the open record: usn_sum, usn_peak, n_nonfinite and the maxima so far
  double w[2];                 // the high cut's one-pole per channel
};

struct WsActArgs {
  long long f0, f1;            // the call's audio frames
  int ch;                      // 1 or 2: the audio is interleaved
  int cmask;                   // control ring length - 1 (a power of two)
  double alpha;                // 1 - exp(-2 pi highcut_hz / 48000)
  double drop;                 // 1 - g_floor
};

// ---- detector ----
// base + s stride + off: sample n0 of stream s.  part[s pmax + (j - n0 / Q)].
__global__ __launch_bounds__(kWsT) void k_ws_usn(const float *__restrict__ base, long long stride, int off,
                                                 const float *__restrict__ hist, const double *__restrict__ h, long long n0,
                                                 long long n1, int pmax, WsPart *__restrict__ part) {
  constexpr int T = kWsT, R = kWsTaps - 1;
  __shared__ float xs[kWsQ + R];
  __shared__ double r_a[T];
  __shared__ unsigned r_n[T];
  const int tid = threadIdx.x, s = blockIdx.y;
  const long long j = n0 / kWsQ + blockIdx.x;
  const long long lo = j * kWsQ > n0 ? j * kWsQ : n0, hi = (j + 1) * kWsQ < n1 ? (j + 1) * kWsQ : n1;
  const int len = (int)(hi - lo);
  const float *x = base + (long long)s * stride + off;
  unsigned nnon = 0;
  // the samples [lo - 62, hi), cleaned, at xs[p - lo + 62]
  for (int i = tid; i < len + R; i += T) {
    const long long p = lo - R + i;
    float v = 0.f;
    if (p >= n0) v = x[p - n0];
    else if (p >= 0) v = hist[(size_t)s * kWsHist + (p & (kWsHist - 1))];
    const bool fin = isfinite(v);
    if (i >= R && !fin) nnon++;
    xs[i] = fin ? v : 0.f;
  }
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < kWsQ / T; q++) {
    const int i = tid + q * T;
    if (i < len) {
      const float *w = &xs[i + R];             // w[-k] = x[n - k]
      double y = 0.0;
#pragma unroll
      for (int k = 0; k < kWsTaps; k++) y += h[k] * (double)w[-k];
      acc += y * y;
    }
  }
  // a fixed tree over the threads
  r_a[tid] = acc; r_n[tid] = nnon;
  __syncthreads();
  for (int st = T / 2; st > 0; st >>= 1) {
    if (tid < st) { r_a[tid] += r_a[tid + st]; r_n[tid] += r_n[tid + st]; }
    __syncthreads();
  }
  if (tid == 0) {
    WsPart q;
    q.sumsq = r_a[0]; q.nnon = r_n[0]; q.pad = 0;
    part[(size_t)s * pmax + blockIdx.x] = q;
  }
}

// ---- control ----
// lane i's value in every lane (i uniform): two readlanes, no LDS
__device__ __forceinline__ double ws_lane(double v, int i) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), i), hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
  return __hiloint2double(hi, lo);
}

// One wave per stream = blockIdx.x.  ctl[s (cmask + 1) + (j & cmask)], ring[s L + (index mod L)].
__global__ __launch_bounds__(64) void k_ws_control(const WsPart *__restrict__ part, int pmax, long long n0, long long n1, WsCoef k,
                                                   WsState *__restrict__ state, WsCtl *__restrict__ ctl, int cmask,
                                                   WsRec *__restrict__ ring, const float *__restrict__ base, long long stride,
                                                   int off, float *__restrict__ hist) {
  const int lane = threadIdx.x, s = blockIdx.x;
  WsState *st = state + s;
  const WsPart *pp = part + (size_t)s * pmax;
  const long long j0 = n0 / kWsQ, jd = n1 / kWsQ;      // first interval the call touches; intervals complete after it
  const bool head_open = n0 > j0 * kWsQ;                // interval j0 began in an earlier call
  double sprev = st->s;
  const double osum = head_open ? st->open_sum : 0.0;
  const unsigned onon = head_open ? st->open_non : 0u;
  WsRec o = st->open;
  int rpos = (int)(j0 % k.R);                           // position of interval jb + i in its record
  long long rec = j0 / k.R;
  for (long long jb = j0; jb < jd; jb += 64) {
    const long long j = jb + lane;
    const int cnt = (int)(jd - jb < 64 ? jd - jb : 64);
    double u = 0.0;
    unsigned non = 0;
    if (lane < cnt) {
      const WsPart q = pp[j - j0];
      double sum = q.sumsq;
      non = q.nnon;
      if (j == j0) { sum = osum + sum; non += onon; }   // on top of the carried open partial, in sample order
      u = sum / (double)kWsQ;
    }
    // the serial chain: one compare, one select, two dependent operations per interval
    double sl = 0.0;
    for (int i = 0; i < cnt; i++) {
      const double ui = ws_lane(u, i);
      const double c = ui > sprev ? k.c_att : k.c_rel;
      sprev = sprev + c * (ui - sprev);
      if (lane == i) sl = sprev;
    }
    // per lane, outside the chain
    const double D = 10.0 * log10(sl);
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      double v = 0.0;
      if (k.on[a]) {
        v = (D - k.lo[a]) / (k.hi[a] - k.lo[a]);
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
      }
      t[a] = v;
    }
    if (lane < cnt) {
      WsCtl c;
      c.t[0] = t[0]; c.t[1] = t[1]; c.t[2] = t[2];
      ctl[(size_t)s * (cmask + 1) + (size_t)(j & cmask)] = c;
    }
    // the records, in interval order
    for (int i = 0; i < cnt; i++) {
      const double ui = ws_lane(u, i), si = ws_lane(sl, i);
      const double tb = ws_lane(t[0], i), th = ws_lane(t[1], i), tm = ws_lane(t[2], i);
      const unsigned ni = (unsigned)__builtin_amdgcn_readlane((int)non, i);
      if (rpos == 0) { o.usn_sum = 0.0; o.usn_peak = 0.0; o.max_blend = 0.0; o.max_highcut = 0.0; o.max_mute = 0.0; o.n_nonfinite = 0; }
      o.usn_sum += ui;
      o.usn_peak = fmax(o.usn_peak, ui);
      o.max_blend = fmax(o.max_blend, tb); o.max_highcut = fmax(o.max_highcut, th); o.max_mute = fmax(o.max_mute, tm);
      o.n_nonfinite += ni;
      if (++rpos == k.R) {
        o.index = (uint64_t)rec;
        o.first_interval = (uint64_t)(rec * k.R);
        o.n_intervals = (uint32_t)k.R;
        o.smoothed = si; o.t_blend = tb; o.t_highcut = th; o.t_mute = tm;
        if (lane == 0) ring[(size_t)s * k.L + (size_t)(rec % k.L)] = o;
        rpos = 0; rec++;
      }
    }
  }
  if (lane == 0) {
    st->s = sprev;
    st->open = o;
    if (n1 > jd * kWsQ) {                               // the call ends inside interval jd: its piece stays open
      const WsPart q = pp[jd - j0];
      st->open_sum = (jd == j0 ? osum : 0.0) + q.sumsq;
      st->open_non = (jd == j0 ? onon : 0u) + q.nnon;
    } else {
      st->open_sum = 0.0;
      st->open_non = 0u;
    }
  }
  // the call's last 63 samples to the carry (the partials are done: k_ws_usn ran in front of this kernel)
  if (lane < kWsHist - 1) {
    const long long p = n1 - (kWsHist - 1) + lane;
    if (p >= n0) hist[(size_t)s * kWsHist + (p & (kWsHist - 1))] = base[(long long)s * stride + off + (p - n0)];
  }
}

// ---- action ----
// the control values chunk g ramps between: those of interval g - 2 at its start, of g - 1 at its end (0 below interval 0)
struct WsRamp { double v0[3], d[3]; };
__device__ __forceinline__ WsRamp ws_ramp(const WsCtl *__restrict__ c, int cmask, long long g) {
  WsRamp r;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double v0 = g >= 2 ? c[(g - 2) & cmask].t[a] : 0.0, v1 = g >= 1 ? c[(g - 1) & cmask].t[a] : 0.0;
    r.v0[a] = v0;
    r.d[a] = v1 - v0;
  }
  return r;
}

// Frames [lo, hi) of chunk g of stream s: f(i, p, x1) per frame with i = f - lo, p the ramp position and x1 the blended
// channels (a mono chain: its one channel as it is).
template <class F>
__device__ __forceinline__ void ws_walk(const double *x, const WsActArgs &a, const WsRamp &r, long long g, long long lo,
                                        long long hi, F &&f) {
  const double *px = x + (lo - a.f0) * a.ch;
  const int n = (int)(hi - lo), i0 = (int)(lo - g * kWsA);
  for (int i = 0; i < n; i++) {
    const double p = (double)(i0 + i + 1) / (double)kWsA;
    double x1[2];
    if (a.ch == 2) {
      const double L = px[2 * i], R = px[2 * i + 1];
      const double tb = r.v0[0] + p * r.d[0];
      const double S = 0.5 * (L - R);
      x1[0] = L - tb * S;
      x1[1] = R + tb * S;
    } else {
      x1[0] = px[i];
      x1[1] = 0.0;
    }
    f(i, p, x1);
  }
}

__device__ __forceinline__ void ws_chunk(const WsActArgs &a, int run, long long &g, long long &lo, long long &hi) {
  g = a.f0 / kWsA + run;
  lo = g * kWsA > a.f0 ? g * kWsA : a.f0;
  hi = (g + 1) * kWsA < a.f1 ? (g + 1) * kWsA : a.f1;
}

// Lane = chunk `run` of stream blockIdx.y; the call's audio of stream s at aud + s astride (frame f0 first).
// G[(s 2 + c) rmax + run]: the chunk's end state of channel c from the zero state.
__global__ __launch_bounds__(64) void k_ws_pass1(const double *__restrict__ aud, long long astride, WsActArgs a,
                                                 const WsCtl *__restrict__ ctl, int runs, int rmax, double *__restrict__ G) {
  const int run = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (run >= runs) return;
  long long g, lo, hi;
  ws_chunk(a, run, g, lo, hi);
  const WsRamp r = ws_ramp(ctl + (size_t)s * (a.cmask + 1), a.cmask, g);
  double w0 = 0.0, w1 = 0.0;
  ws_walk(aud + (long long)s * astride, a, r, g, lo, hi, [&](int, double, const double *x1) {
    w0 = w0 + a.alpha * (x1[0] - w0);
    w1 = w1 + a.alpha * (x1[1] - w1);
  });
  G[((size_t)s * 2 + 0) * rmax + run] = w0;
  G[((size_t)s * 2 + 1) * rmax + run] = w1;
}

// z <- beta^n z with the table pw[b] = beta^(2^b)
__device__ __forceinline__ double ws_bpow(const double *__restrict__ pw, unsigned n, double z) {
  for (int b = 0; n != 0u && b < kWsPow; b++, n >>= 1)
    if (n & 1u) z = pw[b] * z;
  return z;
}

__device__ __forceinline__ int ws_len(const WsActArgs &a, int run) {
  long long g, lo, hi;
  ws_chunk(a, run, g, lo, hi);
  return (int)(hi - lo);
}

// One wave per (stream, channel) = blockIdx.x: the start state of every chunk of the call from the carried w.
__global__ __launch_bounds__(64) void k_ws_nodes(const double *__restrict__ G, double *__restrict__ start, WsActArgs a, int runs,
                                                 int rmax, const double *__restrict__ pw, const WsState *__restrict__ state) {
  const int s = blockIdx.x / a.ch, c = blockIdx.x - s * a.ch, lane = threadIdx.x;
  const size_t row = ((size_t)s * 2 + c) * rmax;
  const double *g = G + row;
  double *o = start + row;
  const int K = (runs + 63) / 64;
  const int r0 = lane * K < runs ? lane * K : runs, r1 = r0 + K < runs ? r0 + K : runs;
  // my chunks folded from the zero state: (n, q)
  double q = 0.0;
  int n = 0;
  for (int r = r0; r < r1; r++) {
    const int len = ws_len(a, r);
    q = ws_bpow(pw, (unsigned)len, q) + g[r];
    n += len;
  }
  // inclusive scan inside the wave: (pn, pq) then (n, q) is (pn + n, beta^n pq + q)
#pragma unroll
  for (int lv = 0; lv < 6; lv++) {
    const int o_ = 1 << lv;
    const double p = __shfl_up(q, o_, 64);
    const int pn = __shfl_up(n, o_, 64);
    if (lane >= o_) {
      q = ws_bpow(pw, (unsigned)n, p) + q;
      n += pn;
    }
  }
  double e = __shfl_up(q, 1, 64);
  int en = __shfl_up(n, 1, 64);
  if (lane == 0) { e = 0.0; en = 0; }
  double x = ws_bpow(pw, (unsigned)en, state[s].w[c]) + e;
  for (int r = r0; r < r1; r++) {
    o[r] = x;
    x = ws_bpow(pw, (unsigned)ws_len(a, r), x) + g[r];
  }
}

// Lane = chunk as in pass 1: the chunk from its start state, stored in place.  The call's last chunk leaves the carry.
__global__ __launch_bounds__(64) void k_ws_pass2(double *aud, long long astride, WsActArgs a,
                                                 const WsCtl *__restrict__ ctl, int runs, int rmax,
                                                 const double *__restrict__ start, WsState *__restrict__ state) {
  const int run = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (run >= runs) return;
  long long g, lo, hi;
  ws_chunk(a, run, g, lo, hi);
  const WsRamp r = ws_ramp(ctl + (size_t)s * (a.cmask + 1), a.cmask, g);
  double w0 = start[((size_t)s * 2 + 0) * rmax + run], w1 = a.ch == 2 ? start[((size_t)s * 2 + 1) * rmax + run] : 0.0;
  double *out = aud + (long long)s * astride + (lo - a.f0) * a.ch;
  ws_walk(aud + (long long)s * astride, a, r, g, lo, hi, [&](int i, double p, const double *x1) {
    const double th = r.v0[1] + p * r.d[1], tm = r.v0[2] + p * r.d[2];
    const double gain = 1.0 - tm * a.drop;
    w0 = w0 + a.alpha * (x1[0] - w0);
    const double y0 = x1[0] + th * (w0 - x1[0]);
    if (a.ch == 2) {
      w1 = w1 + a.alpha * (x1[1] - w1);
      const double y1 = x1[1] + th * (w1 - x1[1]);
      out[2 * i] = gain * y0;
      out[2 * i + 1] = gain * y1;
    } else {
      out[i] = gain * y0;
    }
  });
  if (run == runs - 1) { state[s].w[0] = w0; state[s].w[1] = w1; }
}

}  // namespace fmr
