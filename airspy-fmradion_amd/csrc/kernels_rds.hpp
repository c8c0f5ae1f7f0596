// kernels_rds.hpp -- the device part of the RDS decoder (fmr_create_rds).
//
// Input: the demodulated MPX of an FM stream at 384 kHz (the chain's base slot, floats), call by call.  Output: hard bits
// after differential decoding, one per RDS symbol, with the symbol's position, written to page-locked host memory; the
// block synchronisation and group assembly run on the host (host/fmradion_rds.hpp).
//
// Everything is indexed by ABSOLUTE positions counted from the chain's first MPX sample, so the result does not depend
// on how the signal is cut into calls:
//   n  MPX sample (384 kHz)
//   m  decimated sample (24 kHz): y[m] belongs to n = 16 m; the carrier table is indexed by (19 n) mod 128, since
//      57000 / 384000 = 19 / 128 cycles per sample: exact, nothing accumulates phase
//   U  1/19 of an MPX sample: one RDS symbol (57000 / 48 = 1187.5 Hz) lasts exactly 6144 U (6144 / 19 samples), so the
//      symbol clock is an integer in U and never drifts
//   w  window of 64 symbol periods: [64 w 6144, 64 (w + 1) 6144) U
//
// Stages of one call (one stream per grid row):
//   k_rds_mix    y1[m] = sum_k h1[k] x[16 m - k] lo[(19 (16 m - k)) mod 128]: mix 57 kHz to DC, 128-tap low-pass, keep 1 in 16
//   k_rds_mf     y2[m] = sum_j h2[j] y1[m - j]: the standard's cos shaping (81 taps at 24 kHz) as the matched filter
//   k_rds_halo   the last 256 MPX samples, for the next call's k_rds_mix
//   k_rds_est    per complete window: the symbol timing that maximises the biphase matched-filter energy over 64
//                candidate phases (parabolic refinement), and sum s^2 of the soft symbols at that timing
//   k_rds_scan   one lane per stream walks the call's windows: keeps the timing continuous, unwraps the carrier phase
//                arg(sum s^2) / 2 modulo pi against a tracked frequency term, assigns the symbols to windows
//   k_rds_bits   per window: soft biphase symbol s = y2(start) - y2(mid) at the scan's timing, decision variable
//                d = Re(s e^{-i theta}), hard bit of its sign, differential decoding (the pi ambiguity of the carrier
//                cancels), and the reliability rho = d / sqrt(window energy) of every symbol, out to host memory
// A non-finite MPX sample is read as 0: nothing non-finite reaches an estimate or a bit.  y1 and y2 live in per-stream
// rings of R (a power of two) samples indexed by m mod R; a ring holds the call plus four windows of history.
#pragma once
#include <hip/hip_runtime.h>

namespace fmr {

constexpr int kRdsD = 16;               // 384 kHz -> 24 kHz
constexpr int kRdsNT1 = 128;            // taps of the mixing low-pass
constexpr int kRdsNT2 = 81;             // taps of the matched filter (+- 2 symbols at 24 kHz)
constexpr int kRdsHalo = 256;           // MPX history ring (> kRdsNT1)
constexpr long long kRdsSym = 6144;     // one symbol in U (1/19 sample)
constexpr int kRdsWin = 64;             // symbols per window
constexpr int kRdsCand = 64;            // timing candidates per symbol period (96 U apart)
constexpr int kRdsMaxSym = 72;          // bit slots per window in the hand-off (a window carries 63 .. 65 symbols)
// MPX time of y2[i]: 16 (i - 40) - 63.5 samples (the two filters' delays): y2 index of MPX time T is (T + 63.5) / 16 + 40
constexpr double kRdsDelay1 = 63.5, kRdsDelay2 = 40.0;

struct RdsRec {            // one window as the scan decided it
  long long k_first;       // first symbol (absolute symbol number) ...
  long long tau;           // ... symbol k starts at k 6144 + tau  [U]
  double kmid;             // symbol the carrier phase refers to
  float theta, fr;         // carrier phase at kmid and its slope [rad / symbol]
  float energy;            // mean |s|^2 of the window
  int count, valid;        // symbols of the window; 0: no window yet
  int pad;
};

struct RdsState {          // carried from call to call, written by k_rds_scan only
  double tau, theta, fr, level;
  long long k_next, nwin;
  RdsRec prev;
};

struct RdsEst {            // k_rds_est's result for one window
  float phi, e_best, s2x, s2y, eabs;
  float pad[3];
};

struct RdsSlotHdr {        // per stream, in front of the records and bits of a call in the host hand-off
  int nw, pad;
  float tau_samples, theta, freq_hz, level;    // the scan's estimates after the call's last window
  float timing_frac, pad2;                     // timing within a symbol [symbols]
};

// A stream's part of a host slot: RdsSlotHdr, max_w RdsRec, max_w x kRdsMaxSym bits (bytes), then max_w x
// (kRdsMaxSym + 1) reliabilities (floats): per window the symbol before its first (the one the differential decoding
// reads, under the window before's record) and then its symbols.
__host__ __device__ inline size_t rds_slot_bits_off(int max_w) { return sizeof(RdsSlotHdr) + sizeof(RdsRec) * (size_t)max_w; }
__host__ __device__ inline size_t rds_slot_rho_off(int max_w) { return rds_slot_bits_off(max_w) + (size_t)kRdsMaxSym * max_w; }
__host__ __device__ inline size_t rds_slot_bytes(int max_w) {
  return rds_slot_rho_off(max_w) + sizeof(float) * (size_t)(kRdsMaxSym + 1) * max_w;
}

__device__ __forceinline__ float rds_fin(float v) { return isfinite(v) ? v : 0.f; }

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_rds_mix(const float *__restrict__ base, long long base_stride, int base_off,
                                                   const float *__restrict__ xhalo, long long n0, long long m0, int cnt,
                                                   const float *__restrict__ h1, const float2 *__restrict__ lo,
                                                   float2 *__restrict__ y1, int R) {
  const int s = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= cnt) return;
  const long long m = m0 + i, nc = kRdsD * m;       // (nc < n0 + N: the host counts only outputs whose input is there)
  const float *x = base + (long long)s * base_stride + base_off;
  const float *hx = xhalo + (long long)s * kRdsHalo;
  float ar = 0.f, ai = 0.f;
  for (int k = 0; k < kRdsNT1; k++) {
    const long long n = nc - k;
    if (n < 0) break;
    const float v = n >= n0 ? x[n - n0] : hx[n & (kRdsHalo - 1)];
    const float hv = h1[k] * rds_fin(v);
    const float2 c = lo[(19 * (int)(n & 127)) & 127];
    ar = fmaf(hv, c.x, ar);
    ai = fmaf(hv, c.y, ai);
  }
  y1[(long long)s * R + (m & (R - 1))] = make_float2(ar, ai);
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_rds_mf(const float2 *__restrict__ y1, float2 *__restrict__ y2, int R, long long m0,
                                                  int cnt, const float *__restrict__ h2) {
  const int s = blockIdx.y, i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= cnt) return;
  const long long m = m0 + i;
  const float2 *r = y1 + (long long)s * R;
  float ar = 0.f, ai = 0.f;
  for (int j = 0; j < kRdsNT2; j++) {
    if (m - j < 0) break;
    const float2 v = r[(m - j) & (R - 1)];
    ar = fmaf(h2[j], v.x, ar);
    ai = fmaf(h2[j], v.y, ai);
  }
  y2[(long long)s * R + (m & (R - 1))] = make_float2(ar, ai);
}

// the last kRdsHalo MPX samples up to n0 + N (older ring entries stay: they are still the history of a short call)
__global__ __launch_bounds__(kRdsHalo) void k_rds_halo(const float *__restrict__ base, long long base_stride, int base_off,
                                                      float *__restrict__ xhalo, long long n0, int N) {
  const int s = blockIdx.x, t = threadIdx.x;
  const long long n = n0 + N - kRdsHalo + t;
  if (n < n0) return;
  xhalo[(long long)s * kRdsHalo + (n & (kRdsHalo - 1))] = rds_fin(base[(long long)s * base_stride + base_off + (n - n0)]);
}

// y2 at MPX time pos U (Catmull-Rom between the 24 kHz samples)
__device__ __forceinline__ float2 rds_at(const float2 *__restrict__ r, int R, long long pos) {
  const double fi = ((double)pos / 19.0 + kRdsDelay1) / kRdsD + kRdsDelay2;
  const double fl = floor(fi);
  const long long i0 = (long long)fl;
  const float u = (float)(fi - fl);
  float2 p[4];
  for (int j = 0; j < 4; j++) p[j] = (i0 - 1 + j >= 0) ? r[(i0 - 1 + j) & (R - 1)] : make_float2(0.f, 0.f);
  const float u2 = u * u, u3 = u2 * u;
  const float c0 = -0.5f * u3 + u2 - 0.5f * u, c1 = 1.5f * u3 - 2.5f * u2 + 1.f, c2 = -1.5f * u3 + 2.f * u2 + 0.5f * u,
              c3 = 0.5f * u3 - 0.5f * u2;
  return make_float2(c0 * p[0].x + c1 * p[1].x + c2 * p[2].x + c3 * p[3].x, c0 * p[0].y + c1 * p[1].y + c2 * p[2].y + c3 * p[3].y);
}

// soft biphase symbol starting at pos: the doublet's first half minus its second
__device__ __forceinline__ float2 rds_soft(const float2 *__restrict__ r, int R, long long pos) {
  const float2 a = rds_at(r, R, pos), b = rds_at(r, R, pos + kRdsSym / 2);
  return make_float2(a.x - b.x, a.y - b.y);
}

// grid (nw, S), 64 lanes: lane c = timing candidate c 96 U, then lane k = symbol k of the window at the chosen timing
__global__ __launch_bounds__(64) void k_rds_est(const float2 *__restrict__ y2, int R, long long w0, RdsEst *__restrict__ est,
                                                int max_w) {
  __shared__ float e[kRdsCand];
  __shared__ float red[3][kRdsWin];
  const int wl = blockIdx.x, s = blockIdx.y, c = threadIdx.x;
  const long long w = w0 + wl;
  const float2 *r = y2 + (long long)s * R;
  const long long j0 = w * kRdsWin;
  // The stream's first symbol period is left out of the timing: its symbol is cut by the start of the stream (its pulse
  // reaches back before sample 0), or, for the candidates past a symbol that starts late in the period, not there at all,
  // so the candidates on either side of that symbol would be compared over different symbols (up to 3.7 samples of bias).
  // (The sums for the phase and the level below keep it: there a cut symbol only weighs less, it has the phase of the
  // others, and the scan smooths the level.)
  const int k_lo = w == 0 ? 1 : 0;
  float acc = 0.f;
  for (int k = k_lo; k < kRdsWin; k++) {
    const float2 v = rds_soft(r, R, (j0 + k) * kRdsSym + (long long)c * (kRdsSym / kRdsCand));
    acc += v.x * v.x + v.y * v.y;
  }
  e[c] = acc;
  __syncthreads();
  int best = 0;
  for (int q = 1; q < kRdsCand; q++) if (e[q] > e[best]) best = q;     // (every lane reaches the same answer)
  const float em = e[(best + kRdsCand - 1) % kRdsCand], e0 = e[best], ep = e[(best + 1) % kRdsCand];
  const float den = em - 2.f * e0 + ep;
  const float d = den < 0.f ? fminf(fmaxf(0.5f * (em - ep) / den, -0.5f), 0.5f) : 0.f;
  float phi = ((float)best + d) * (float)(kRdsSym / kRdsCand);
  if (phi < 0.f) phi += (float)kRdsSym;
  if (phi >= (float)kRdsSym) phi -= (float)kRdsSym;
  const float2 v = rds_soft(r, R, (j0 + c) * kRdsSym + (long long)rintf(phi));
  red[0][c] = v.x * v.x - v.y * v.y;
  red[1][c] = 2.f * v.x * v.y;
  red[2][c] = v.x * v.x + v.y * v.y;
  __syncthreads();
  if (c == 0) {
    float a = 0.f, b = 0.f, q = 0.f;
    for (int k = 0; k < kRdsWin; k++) { a += red[0][k]; b += red[1][k]; q += red[2][k]; }
    est[(long long)s * max_w + wl] = RdsEst{phi, e0, a, b, q / kRdsWin, {0.f, 0.f, 0.f}};
  }
}

// one lane per stream: the windows of the call in order.  rec[s][0] = the window before the call's first (carried),
// rec[s][1 + i] = window w0 + i.
__global__ void k_rds_scan(const RdsEst *__restrict__ est, int nw, long long w0, int max_w, RdsState *__restrict__ st,
                           RdsRec *__restrict__ rec, char *__restrict__ slot, size_t slot_stride, int S) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  RdsState z = st[s];
  RdsRec *rs = rec + (long long)s * (max_w + 1);
  rs[0] = z.prev;
  constexpr double P = (double)kRdsSym, PI = 3.14159265358979323846;
  for (int i = 0; i < nw; i++) {
    const RdsEst e = est[(long long)s * max_w + i];
    const long long w = w0 + i;
    const double th_raw = 0.5 * atan2((double)e.s2y, (double)e.s2x);
    if (z.nwin == 0) {
      z.tau = e.phi; z.theta = th_raw; z.fr = 0.0; z.level = e.eabs;
      z.k_next = (long long)ceil(((double)w * kRdsWin * P - z.tau) / P);
    } else if (e.eabs >= 0.05 * z.level) {
      double d = (double)e.phi - z.tau;
      d -= P * rint(d / P);                                // nearest representative: the timing stays continuous
      z.tau += 0.5 * d;
      const double pred = z.theta + z.fr * kRdsWin;
      // th_raw is the phase at the mean start of the estimate's 64 symbols, (64 w + 31.5) P + phi; kmid names the
      // window's centre, (64 w + 32) P: carry the phase there along the tracked slope (at 3 Hz up to 8 mrad)
      const double th_c = th_raw + z.fr * (0.5 - (double)e.phi / P);
      const double th = th_c + PI * rint((pred - th_c) / PI);       // modulo pi: differential decoding cancels pi
      z.fr += 0.5 * ((th - z.theta) / kRdsWin - z.fr);
      z.theta = th;
    } else {                                               // a dropout: hold the timing, let the phase run on
      z.theta += z.fr * kRdsWin;
    }
    z.level += 0.25 * (e.eabs - z.level);
    const long long tau_i = (long long)llrint(z.tau);
    const long long k_end = (long long)ceil(((double)(w + 1) * kRdsWin * P - (double)tau_i) / P);
    long long count = k_end - z.k_next;
    count = count < 0 ? 0 : count > kRdsMaxSym ? kRdsMaxSym : count;
    RdsRec r{};
    r.k_first = z.k_next; r.tau = tau_i;
    r.kmid = ((double)(w * kRdsWin + kRdsWin / 2) * P - (double)tau_i) / P;
    r.theta = (float)z.theta; r.fr = (float)z.fr;
    r.energy = e.eabs; r.count = (int)count; r.valid = 1;
    rs[i + 1] = r;
    z.k_next += count;
    z.prev = r;
    z.nwin++;
  }
  st[s] = z;
  double tf = fmod(z.tau, P);
  if (tf < 0) tf += P;
  *reinterpret_cast<RdsSlotHdr *>(slot + (size_t)s * slot_stride) =
      RdsSlotHdr{nw, 0, (float)(z.tau / 19.0), (float)z.theta, (float)(z.fr * 1187.5 / (2.0 * PI)), (float)z.level,
                 (float)(tf / P), 0.f};
}

// decision variable of symbol k under record r: Re(s e^{-i phase}), phase = theta + fr (k - kmid); the hard decision is
// its sign
__device__ __forceinline__ float rds_decide(const float2 *__restrict__ y, int R, const RdsRec &r, long long k) {
  const float2 v = rds_soft(y, R, k * kRdsSym + r.tau);
  const float ph = r.theta + r.fr * (float)((double)k - r.kmid);
  float sn, cs;
  sincosf(ph, &sn, &cs);
  return v.x * cs + v.y * sn;
}

// reliability of a decision: d in units of the record's rms symbol level (0 where the window carried nothing)
__device__ __forceinline__ float rds_rho(float d, const RdsRec &r) {
  return r.energy > 0.f ? rds_fin(d / sqrtf(r.energy)) : 0.f;
}

// grid (nw, S), 128 lanes: bits and reliabilities of window wl (one symbol per lane); records, bits and reliabilities go
// to the host slot of the call
__global__ __launch_bounds__(128) void k_rds_bits(const float2 *__restrict__ y2, int R, const RdsRec *__restrict__ rec,
                                                  int max_w, char *__restrict__ slot, size_t slot_stride) {
  __shared__ int hs[kRdsMaxSym + 1];
  const int wl = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  const RdsRec *rs = rec + (long long)s * (max_w + 1);
  const RdsRec r = rs[wl + 1];
  const float2 *y = y2 + (long long)s * R;
  char *sl = slot + (size_t)s * slot_stride;
  RdsRec *hrec = reinterpret_cast<RdsRec *>(sl + sizeof(RdsSlotHdr));
  unsigned char *bits = reinterpret_cast<unsigned char *>(sl + rds_slot_bits_off(max_w)) + (size_t)wl * kRdsMaxSym;
  float *rho = reinterpret_cast<float *>(sl + rds_slot_rho_off(max_w)) + (size_t)wl * (kRdsMaxSym + 1);
  if (t < r.count) {                                        // (count <= kRdsMaxSym: the scan clamps it)
    const float d = rds_decide(y, R, r, r.k_first + t);
    hs[t + 1] = d < 0.f ? 1 : 0;
    rho[t + 1] = rds_rho(d, r);
  }
  if (t == 0) {
    const RdsRec p = rs[wl];                                // the window before (of this call, or carried)
    const bool have = p.valid && p.count > 0;
    const float d = have ? rds_decide(y, R, p, r.k_first - 1) : 0.f;
    hs[0] = d < 0.f ? 1 : 0;
    rho[0] = have ? rds_rho(d, p) : 0.f;
    hrec[wl] = r;
  }
  __syncthreads();
  if (t < r.count) bits[t] = (unsigned char)(hs[t + 1] ^ hs[t]);
}

}  // namespace fmr
