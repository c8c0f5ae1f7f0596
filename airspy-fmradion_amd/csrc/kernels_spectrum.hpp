// kernels_spectrum.hpp -- Welch power spectrum of IQ rows (fmr_spectrum_*).
//
// Segment j of a row covers the absolute samples [j H, j H + N) and is processed in the call that delivers its last
// sample.  Per segment:  P_j[k] = |sum_n w[n] x_j[n] exp(-2 pi i k n / N)|^2  (fp32), then per bin
//     sum[k] += P_j[k]  (fp64)      max[k] = max(max[k], P_j[k])  (fp32)
// over the segments that hold no non-finite sample.  The density scaling 1 / (F sum w^2), the division by the count and
// the fftshift happen on the host when the result is read.
//
// k_spec_seg: one workgroup = one contiguous run of segments of one row.  Per segment it loads the N samples (from the
// call's input, or from the row's ring of the last N samples of earlier calls), converts the raw formats with the front
// end's rule (fmr::iq_load1), multiplies by the window and stores them BIT-REVERSED into LDS; then log2 N radix-2 / radix-4
// decimation-in-time passes run in place (each thread owns whole butterflies: one barrier per pass), the output lands in
// natural order, and every thread folds the power of its bins into registers (fp64 sum, fp32 max) across the run.  The
// per-segment arithmetic does not depend on where a segment falls in a call (the peak hold is bit-identical for any
// cut).  Only the run's partial sums go to HBM; k_spec_reduce adds them in run order into the row's accumulators (no
// float atomics) and refreshes the ring.
//
// The LDS padding and the sub-block partition are the Welch segment engine's (kernels_welch.hpp); the passes are
// welch_fft's arithmetic, written out in this kernel.
// N = 16384 needs 132 KiB of LDS: one workgroup per CU; N <= 8192 fits two.
// Twiddles tw[i] = exp(-2 pi i i / N) and the window are built on the host in double and rounded once to fp32.
//
// Waterfall (fmr_spectrum_create_waterfall; k_spec_seg<.., WF = true> and k_spec_lines).  Line l of a row is made of the
// segments [l R, (l + 1) R) (absolute indices); it is complete in the call that delivers the last sample of segment
// (l + 1) R - 1.  MEAN keeps the fp32 sum of the counted segments' P_j[k] and their count c_l, PEAK their maximum; the
// division, the density scaling and the fftshift happen on the host when a line is read.
// Addition order (a function of a segment's index q = j - l R within its line only, never of the call cut or of the
// run partition): the line is cut into sub-blocks of SPEC_WF_SUB segments, sub-block b = q / SPEC_WF_SUB (the last one
// of a line is shorter when SPEC_WF_SUB does not divide R).  Within a sub-block the counted P_j are added one by one in
// segment order, starting from the first (S_b = (..((P_q0 + P_q0+1) + P_q0+2) ..)); the line is
// (..((S_0 + S_1) + S_2) ..) in sub-block order.  A skipped segment adds nothing.
// A workgroup run of the waterfall form never straddles a sub-block boundary: run r of a launch is (the part inside
// the launch of) sub-block g0 + r, sub-blocks numbered g = l ceil(R / SPEC_WF_SUB) + b.  A sub-block cut by the end of a
// call is carried in open_sub / open_cnt and the run that continues it starts from there, so its additions go on in
// the same order.  k_spec_lines (one block column per line the launch touches) combines the sub-block values in order,
// starting from the open line's partial of the launch before, writes complete lines into the ring [row][l mod L][N]
// and their counts beside it, and leaves the open line's partial for the next launch (two copies by launch parity: the
// block that reads the old one is not the block that writes the new one).  The line state lives in registers and HBM:
// the LDS of the segment pass is unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_welch.hpp"

// threads and LDS bytes of k_spec_seg at 2^logn points (host and device: the engine sizes its runs with them)
__host__ __device__ constexpr int spec_threads(int logn) { return (1 << logn) / 4 < 1024 ? (1 << logn) / 4 : 1024; }
__host__ __device__ constexpr int spec_lds_bytes(int logn) { return ((1 << logn) + ((1 << logn) >> 5)) * 8; }

template <int LOGN>
struct SpecShape {
  static constexpr int N = 1 << LOGN;
  static constexpr int T = spec_threads(LOGN);                     // threads: at least one radix-4 butterfly each per pass
  static constexpr int BINS = N / T;                               // bins per thread in the accumulation
  static constexpr int LDS_BYTES = spec_lds_bytes(LOGN);
};

// Waterfall arguments of one launch (by value).  The launch takes the segments [a0, a1) (a0 = k_spec_seg's seg0).
constexpr int SPEC_WF_SUB = 8;                 // segments per sub-block of a line (the addition order above)
struct SpecWf {
  int which;                 // 0 = mean (sum), 1 = peak (max)
  int R, SB;                 // segments per line, sub-blocks per line = ceil(R / SPEC_WF_SUB)
  long long g0, a1;          // sub-block of the launch's first segment; end of the launch's segments
  float *plsub;              // [row * rmax + run][N]: the sub-block's value so far (the carried part included)
  int *plcnt;                // [row * rmax + run]: its counted segments so far
  float *open_sub;           // [row][N], open_cnt [row]: the sub-block a call's end cut
  int *open_cnt;
};

// Row `row` of the call: input at in + row * in_stride (IQ samples of format FMT, in_n of them), ring row at
// ring + row * N (sample p of the stream at ring[p mod N] for p < tb).  Segments seg0 .. seg0 + n_seg - 1 of this call,
// run r = blockIdx.x takes [r per_run, min((r + 1) per_run, n_seg)).  Partials of run r: psum / pmax row (row * rmax + r)
// of N bins, pcnt[row * rmax + r] = (segments counted, segments skipped).
// WF (waterfall form): run r is sub-block wf.g0 + r clipped to the launch's segments [seg0, wf.a1); beside the partials
// above it keeps the sub-block's line value (fp32 sum or maximum in segment order) and writes it to wf.plsub / wf.plcnt.
template <int LOGN, int FMT, bool WF>
__global__ __launch_bounds__(SpecShape<LOGN>::T) void k_spec_seg(
    const void *__restrict__ in, long long in_stride, const float2 *__restrict__ ring, long long tb, long long seg0,
    int n_seg, int per_run, int hop, const float *__restrict__ win, const float2 *__restrict__ tw,
    double *__restrict__ psum, float *__restrict__ pmax, int2 *__restrict__ pcnt, int rmax, SpecWf wf) {
  using S = SpecShape<LOGN>;
  constexpr int N = S::N, T = S::T;
  extern __shared__ float2 lds_sp[];
  const int tid = threadIdx.x;
  const int run = blockIdx.x, row = blockIdx.y;
  int j_lo = run * per_run;
  int j_hi = min(j_lo + per_run, n_seg);
  [[maybe_unused]] float ls[WF ? S::BINS : 1];      // the sub-block's line value of this thread's bins
  [[maybe_unused]] int lcnt = 0;
  if constexpr (WF) {
    long long lo, hi;
    fmr::welch_sub(wf.R, SPEC_WF_SUB, wf.SB, wf.g0 + run, lo, hi);
    const bool carried = lo < seg0;        // the call before ended inside this sub-block (the launch's first run only)
    j_lo = (int)(max(lo, seg0) - seg0);
    j_hi = (int)(min(hi, wf.a1) - seg0);
#pragma unroll
    for (int b = 0; b < S::BINS; b++) ls[b] = carried ? wf.open_sub[(size_t)row * N + tid + b * T] : 0.f;
    if (carried) lcnt = wf.open_cnt[row];
  }
  const unsigned char *inrow = reinterpret_cast<const unsigned char *>(in) + (size_t)row * in_stride * fmr::IqFmt<FMT>::BPS;
  const float2 *ringrow = ring + (size_t)row * N;

  double acc[S::BINS];
  float pk[S::BINS];
#pragma unroll
  for (int b = 0; b < S::BINS; b++) { acc[b] = 0.0; pk[b] = 0.f; }
  int counted = 0, skipped = 0;

  for (int j = j_lo; j < j_hi; j++) {
    const long long p0 = (seg0 + j) * (long long)hop;      // absolute index of the segment's first sample
    int bad = 0;
    for (int i = tid; i < N; i += T) {
      const long long p = p0 + i;
      const float2 v = p < tb ? ringrow[p & (N - 1)] : fmr::iq_load1<FMT>(inrow, p - tb);
      bad |= !(isfinite(v.x) && isfinite(v.y));
      const float w = win[i];
      const int r = (int)(__brev((unsigned)i) >> (32 - LOGN));
      lds_sp[fmr::spec_pad(r)] = make_float2(v.x * w, v.y * w);
    }
    bad = __syncthreads_or(bad);
    if (bad) { skipped++; continue; }      // (uniform: the whole workgroup skips; the next store waits on the barrier above)
    // welch_fft's passes, written out: called as a function they cost this kernel registers (kernels_welch.hpp)
    int span = 1;
    if (LOGN & 1) {                        // one radix-2 pass first when log2 N is odd
      for (int b = tid; b < N / 2; b += T) {
        const int e0 = fmr::spec_pad(2 * b), e1 = fmr::spec_pad(2 * b + 1);
        const float2 a0 = lds_sp[e0], a1 = lds_sp[e1];
        lds_sp[e0] = make_float2(a0.x + a1.x, a0.y + a1.y);
        lds_sp[e1] = make_float2(a0.x - a1.x, a0.y - a1.y);
      }
      span = 2;
      __syncthreads();
    }
    // radix-4 DIT pass: four length-s sub-DFTs at block offsets 0, s, 2s, 3s (in bit-reversed order the residues 0, 2, 1,
    // 3 of the length-4s DFT) -> one length-4s DFT in natural order
    for (; span < N; span *= 4) {
      const int tstep = N / (4 * span);    // twiddle index step: W_{4s}^{jk} = tw[j k N / (4 s)]
#pragma unroll 1                   // (unrolled, N = 8192 spills at 1024 threads' 128 VGPRs)
      for (int q = 0; q < N / 4 / T; q++) {
        const int b = tid + q * T;
        const int jj = b & (span - 1);
        const int base = (b - jj) * 4 + jj;
        const int e0 = fmr::spec_pad(base), e1 = fmr::spec_pad(base + 2 * span), e2 = fmr::spec_pad(base + span),
                  e3 = fmr::spec_pad(base + 3 * span);
        const float2 a0 = lds_sp[e0];
        const float2 a1 = fmr::cmul(lds_sp[e1], tw[jj * tstep]);
        const float2 a2 = fmr::cmul(lds_sp[e2], tw[2 * jj * tstep]);
        const float2 a3 = fmr::cmul(lds_sp[e3], tw[3 * jj * tstep]);
        const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
        const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
        // X0 = s02 + s13, X2 = s02 - s13, X1 = d02 - i d13, X3 = d02 + i d13
        lds_sp[fmr::spec_pad(base)] = make_float2(s02.x + s13.x, s02.y + s13.y);
        lds_sp[fmr::spec_pad(base + span)] = make_float2(d02.x + d13.y, d02.y - d13.x);
        lds_sp[fmr::spec_pad(base + 2 * span)] = make_float2(s02.x - s13.x, s02.y - s13.y);
        lds_sp[fmr::spec_pad(base + 3 * span)] = make_float2(d02.x - d13.y, d02.y + d13.x);
      }
      __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < S::BINS; b++) {
      const float2 x = lds_sp[fmr::spec_pad(tid + b * T)];
      const float pw = x.x * x.x + x.y * x.y;
      acc[b] += (double)pw;
      pk[b] = fmaxf(pk[b], pw);
      if constexpr (WF) ls[b] = wf.which ? fmaxf(ls[b], pw) : ls[b] + pw;
    }
    counted++;
    __syncthreads();                       // every thread has read its bins before the next segment's stores
  }
  const size_t prow = (size_t)row * rmax + run;
#pragma unroll
  for (int b = 0; b < S::BINS; b++) {
    psum[prow * N + tid + b * T] = acc[b];
    pmax[prow * N + tid + b * T] = pk[b];
  }
  if (tid == 0) pcnt[prow] = make_int2(counted, skipped);
  if constexpr (WF) {
#pragma unroll
    for (int b = 0; b < S::BINS; b++) wf.plsub[prow * N + tid + b * T] = ls[b];
    if (tid == 0) wf.plcnt[prow] = lcnt + counted;
  }
}

// Per row (grid.y) and 64 bins (grid.x): add the runs' partials into the row's accumulators in a fixed order -- wave g of
// the SPEC_RW waves sums its contiguous share of the runs in run order, wave 0 adds the SPEC_RW sums in wave order (no
// float atomics) -- and copy the call's input samples of absolute positions [max(tb, ta - N), ta) into the ring (after
// k_spec_seg on the same stream: it read the ring slots this overwrites).  Thread 0 of the row's first block adds the
// segment counts.
constexpr int SPEC_RW = 16;
template <int FMT>
__global__ __launch_bounds__(64 * SPEC_RW) void k_spec_reduce(
    const double *__restrict__ psum, const float *__restrict__ pmax, const int2 *__restrict__ pcnt, int runs, int rmax,
    int N, double *__restrict__ acc_sum, float *__restrict__ acc_max, unsigned long long *__restrict__ cnt,
    const void *__restrict__ in, long long in_stride, long long tb, long long ta, float2 *__restrict__ ring) {
  __shared__ double s_sum[SPEC_RW][64];
  __shared__ float s_max[SPEC_RW][64];
  const int row = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  if (runs > 0) {                          // (uniform per launch: the barrier below is reached by every thread)
    const int share = (runs + SPEC_RW - 1) / SPEC_RW;
    const int r0 = wv * share, r1 = min(r0 + share, runs);
    double s = 0.0;
    float m = 0.f;
    if (i < N)
      for (int r = r0; r < r1; r++) {
        const size_t pr = (size_t)row * rmax + r;
        s += psum[pr * N + i];
        m = fmaxf(m, pmax[pr * N + i]);
      }
    s_sum[wv][lane] = s;
    s_max[wv][lane] = m;
    __syncthreads();
    if (wv == 0 && i < N) {
      double t = 0.0;
      float mm = 0.f;
      for (int g = 0; g < SPEC_RW; g++) { t += s_sum[g][lane]; mm = fmaxf(mm, s_max[g][lane]); }
      acc_sum[(size_t)row * N + i] += t;
      acc_max[(size_t)row * N + i] = fmaxf(acc_max[(size_t)row * N + i], mm);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      unsigned long long c = 0, k = 0;
      for (int r = 0; r < runs; r++) {
        const int2 v = pcnt[(size_t)row * rmax + r];
        c += (unsigned long long)v.x;
        k += (unsigned long long)v.y;
      }
      cnt[2 * row] += c;
      cnt[2 * row + 1] += k;
    }
  }
  // ring refresh: N positions per row, spread over the row's blocks' threads
  const unsigned char *inrow = reinterpret_cast<const unsigned char *>(in) + (size_t)row * in_stride * fmr::IqFmt<FMT>::BPS;
  for (int q = blockIdx.x * 64 * SPEC_RW + threadIdx.x; q < N; q += gridDim.x * 64 * SPEC_RW) {
    const long long p = ta - N + q;
    if (p >= tb && p >= 0) ring[(size_t)row * N + (p & (N - 1))] = fmr::iq_load1<FMT>(inrow, p - tb);
  }
}

// Waterfall lines of one launch of k_spec_seg<.., WF = true> (same stream, after it).  Block (x = line l0 + blockIdx.x,
// y = row, z = 256 bins); the launch took the segments [a0, wf.a1) in `runs` runs.  The thread of bin i walks the line's
// sub-blocks inside the launch in order: a complete one joins the line value (the first starts it, or the open line's
// partial of the launch before: line_part[par]), one the call's end cut goes to open_sub.  A complete line goes to
// ring[row][l mod L] (unless a later line of the same launch takes that slot: l + L <= last complete line), an open
// one to line_part[par ^ 1].  Thread 0 of the line's first block does the same with the counts.
__global__ __launch_bounds__(256) void k_spec_lines(SpecWf wf, long long a0, int runs, int rmax, int N, int L, int par,
                                                    float *__restrict__ line_part, int *__restrict__ line_cnt,
                                                    float *__restrict__ ring, unsigned *__restrict__ ring_cnt) {
  const int row = blockIdx.y, rows = gridDim.y;
  const int i = blockIdx.z * 256 + threadIdx.x;
  if (i >= N) return;
  const long long l0 = wf.g0 / wf.SB;
  const long long l = l0 + blockIdx.x;
  const long long g_last = wf.g0 + runs - 1;
  const int b_lo = blockIdx.x == 0 ? (int)(wf.g0 - l0 * wf.SB) : 0;
  const int b_hi = (int)min((long long)wf.SB, g_last - l * wf.SB + 1);
  const long long last_done = wf.a1 / wf.R - 1;            // last line complete after this launch
  const bool cnt_thread = i == 0;
  float v = 0.f;
  int c = 0;
  if (b_lo > 0) {
    v = line_part[((size_t)par * rows + row) * N + i];
    if (cnt_thread) c = line_cnt[par * rows + row];
  }
  for (int b = b_lo; b < b_hi; b++) {
    const long long g = l * wf.SB + b;
    const size_t pr = (size_t)row * rmax + (size_t)(g - wf.g0);
    long long lo, hi;
    fmr::welch_sub(wf.R, SPEC_WF_SUB, wf.SB, g, lo, hi);
    const float s = wf.plsub[pr * N + i];
    if (hi <= wf.a1) {
      v = b == 0 ? s : wf.which ? fmaxf(v, s) : v + s;
      if (cnt_thread) c = b == 0 ? wf.plcnt[pr] : c + wf.plcnt[pr];
    } else {                                               // cut by the call's end: the launch's last run
      wf.open_sub[(size_t)row * N + i] = s;
      if (cnt_thread) wf.open_cnt[row] = wf.plcnt[pr];
    }
  }
  if (l <= last_done) {
    if (l + L > last_done) {
      const size_t slot = (size_t)row * L + (size_t)(l % L);
      ring[slot * N + i] = v;
      if (cnt_thread) ring_cnt[slot] = (unsigned)c;
    }
  } else {
    line_part[((size_t)(par ^ 1) * rows + row) * N + i] = v;
    if (cnt_thread) line_cnt[(par ^ 1) * rows + row] = c;
  }
}
