// kernels_par.hpp -- time-parallel forms of the sample-serial recurrences.
//
// The reference runs five recurrences one sample at a time: IF AGC
// (IfSimpleAgc.cpp:42-56), pilot PLL (PilotPhaseLock.cpp:73-151), two
// de-emphasis IIRs (Filter.cpp:172-178) and two DC-block biquads
// (Filter.cpp:243-250).  A GPU lane runs such a loop no faster than a CPU core,
// so a single stream would be bound by one lane.  These kernels restructure the
// recurrences along time instead (MI355X-first: thousands of chunks in flight):
//
//  * de-emphasis: first-order, pole 0.949 -> its memory is < 768 samples at
//    double precision.  Every chunk simply starts 768 samples early from zero
//    state ("warm-up"), no communication.
//  * DC block: linear, long memory -> multiple shooting.  Pass 1 integrates
//    every chunk from zero state, a node pass propagates s' = G + A^C s through
//    the chunk boundaries, pass 2 re-runs every chunk from its true start.
//    Exact for a linear system after one round.
//  * AGC and PLL: nonlinear but contractive -> multiple shooting with Newton
//    updates of the chunk-boundary states.  Every chunk is integrated with
//    exactly the reference's per-sample arithmetic from its current start-state
//    guess, together with the sensitivity dS_end/dS_start; the node pass solves
//    the linearised boundary conditions; iterate until the boundary mismatch is
//    below tolerance (quadratic convergence, 2-6 rounds).  At convergence the
//    trajectory inside a chunk IS the reference's serial arithmetic; only the
//    chunk start states carry the (<= tolerance) iteration residual.  If the
//    iteration does not converge the serial kernels of kernels.hpp run instead.
#pragma once
#include "kernels.hpp"
#include "pll_compose.hpp"

namespace fmr {

struct IterFlags {
  int agc_converged, agc_iters, agc_fallback, pll_converged, pll_iters, pll_fallback;
  float agc_resid; int pad;
  double pll_resid;
  float agc_hist[16];     // residual after each Newton round (diagnostics)
  double pll_hist[16];
  double pll_comp[8];     // last round: residual per state component
  double pll_rhist[16];   // scaled boundary mismatch seen by each round's integration pass
  int pll_ticket, pll_r_accepted;
  int af_converged, af_iters, af_fallback, af_pad;        // AmDecoder's audio AGC (time-parallel form)
  double af_resid;
  unsigned long long pll_resid_bits, pll_comp_bits[8];   // atomicMax accumulators of the running round
};

// broadcast a double from one lane to the whole wave through SGPRs (v_readlane)
__device__ __forceinline__ double readlane_d(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------------------
// De-emphasis by warm-up (LowPassFilterRC::process_inplace, Filter.cpp:214-221)
// ---------------------------------------------------------------------------
#define FMR_DE_WARMUP 768
template <int C>
__global__ void k_deemph_par(const fm_mpx_t *__restrict__ in0 /* MPX */, const double *__restrict__ in1 /* L-R */, long long in_stride,
                             int in_off, double *__restrict__ out0, double *__restrict__ out1, long long out_stride,
                             int out_off, int n, double b0, double a1, int filt0, int filt1) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y, ch = blockIdx.z;
  const int start = t * C;
  if (start >= n) return;
  double *y = (ch ? out1 : out0) + (long long)s * out_stride + out_off;
  const int end = min(start + C, n);
  auto run = [&](auto *x) {
    if (!(ch ? filt1 : filt0)) {
      for (int i = start; i < end; i++) y[i] = (double)x[i];
      return;
    }
    double w = 0.0;
    serial_prefetch<8>(x, start - FMR_DE_WARMUP, start, [&](int, double v) { w = v - a1 * w; });
    serial_prefetch<8>(x, start, end, [&](int i, double v) {
      w = v - a1 * w;
      y[i] = b0 * w;      // b1 == 0
    });
  };
  if (ch) run(in1 + (long long)s * in_stride + in_off);
  else run(in0 + (long long)s * in_stride + in_off);
}

// ---------------------------------------------------------------------------
// De-emphasis fused with audio stage A (integer decimation): one workgroup stages the tile's
// discriminator-rate samples (768 warm-up + (TOUT-1)*D + NA) in LDS, de-emphasises them in place
// and runs the stage-A FIR out of LDS -- the de-emphasised 384 kHz signal never goes to HBM.
// In-tile recurrence w[n] = x[n] - a1 w[n-1] (Filter.cpp:214-221, b1 == 0): every lane owns
// FMR_DE_LPL consecutive samples; (1) zero-state end value per lane, (2) workgroup scan of the
// affine maps (A^LPL, e) -> true start state per lane, (3) the lane replays its samples with the
// reference's arithmetic.  Only the start state goes through the re-associated scan (a few ulp,
// decaying like A^n); the far end of the warm-up starts from 0 (A^768 = 4e-18).
// FIR: acc = fir_step(hA[k], x[top-k], acc), k ascending (the same chain as k_aud_decim, the oracle's tap order).
// ---------------------------------------------------------------------------
// 15, not 16: the workgroup's tile is then 256 x 15 doubles = 30.7 KB, and TWO of them fit beside the five one-wave
// workgroups (18.4 KB each) a PLL integration pass keeps on every compute unit -- with 16 samples per lane (34.8 KB with the
// pad word an even run needs) one did, and the tail stage's first kernel took 172 us beside the PLL's Jacobian pass (75 us
// alone): the tail then ran 30 us into the next front end, whose workgroups -- a whole unit's LDS each -- cannot start while
// a kernel that uses LDS still has workgroups to place (round 6, profiles/r06_fe_start.txt).
#ifndef FMR_DE_LPL
#define FMR_DE_LPL 15
#endif
// lane l's run starts FMR_DE_RUN doubles behind lane l-1's: the stride must be odd (a half-wave's 8-byte accesses then fall
// on 32 different bank pairs), so an even run length takes a pad word and an odd one must NOT
#define FMR_DE_RUN (FMR_DE_LPL | 1)
struct DeScan {
  double pw[7];          // (A^LPL)^(2^j), j = 0..6
  const double *apow;    // (A^LPL)^k, k = 0..64
};
__device__ __forceinline__ int de_idx(int j) { return (FMR_DE_LPL & 1) ? j : j + j / FMR_DE_LPL; }

// NA_T/D_T > 0: compile-time stage-A shape; every lane then owns 4 consecutive outputs and walks their
// 4 accumulation chains over one shared run of NA + 3 D samples (17 LDS reads per output instead of NA).
template <int BLOCK, int NA_T, int D_T>
__global__ __launch_bounds__(BLOCK) void k_deemph_decim(
    const fm_mpx_t *__restrict__ in0 /* MPX */, const double *__restrict__ in1 /* L-R */, long long in_stride, int in_off, int n_if,
    double b0, double a1, DeScan sc, int filt0, int filt1,
    const double *__restrict__ hA, int NA, int D, long long top0, int count, int tout,
    double *__restrict__ y0, double *__restrict__ y1, long long y_stride, int y_off,
    double *__restrict__ dbg0, double *__restrict__ dbg1, long long dbg_stride, int dbg_off, int ch_base) {
  extern __shared__ double de_xs[];
  __shared__ double wave_tot[BLOCK / 64];
  const int s = blockIdx.y, ch = blockIdx.z + ch_base, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m0 = blockIdx.x * tout;
  const int cnt = min(tout, count - m0);
  if (cnt <= 0) return;
  const fm_mpx_t *x0 = in0 + (long long)s * in_stride + in_off;
  const double *x1 = in1 + (long long)s * in_stride + in_off;
  double *dbg = ch ? dbg1 : dbg0;
  const long long lo = top0 + (long long)m0 * D - (NA - 1);
  long long hi = top0 + (long long)(m0 + cnt - 1) * D;
  if (dbg && blockIdx.x == gridDim.x - 1) hi = n_if - 1;    // debug tap: cover the call to its last sample
  const long long r0 = lo - FMR_DE_WARMUP;
  const int n_t = (int)(hi - r0 + 1);                       // <= BLOCK * FMR_DE_LPL (host-checked)
  {   // all FMR_DE_LPL loads of a lane are in flight before the first LDS write (one memory latency per tile)
    double stage[FMR_DE_LPL];
    if (ch) {      // (block-uniform; one loop per input type keeps the loads free of a branch inside the loop)
#pragma unroll
      for (int u = 0; u < FMR_DE_LPL; u++) { const int j = tid + u * BLOCK; stage[u] = (j < n_t) ? x1[r0 + j] : 0.0; }
    } else {
#pragma unroll
      for (int u = 0; u < FMR_DE_LPL; u++) { const int j = tid + u * BLOCK; stage[u] = (j < n_t) ? (double)x0[r0 + j] : 0.0; }
    }
#pragma unroll
    for (int u = 0; u < FMR_DE_LPL; u++) de_xs[de_idx(tid + u * BLOCK)] = stage[u];
  }
  __syncthreads();
  if (ch ? filt1 : filt0) {
    double *mine = de_xs + tid * FMR_DE_RUN;
    double v[FMR_DE_LPL];
#pragma unroll
    for (int i = 0; i < FMR_DE_LPL; i++) v[i] = mine[i];
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < FMR_DE_LPL; i++) e = v[i] - a1 * e;
    // inclusive scan of S_l = A16 S_{l-1} + e_l inside the wave
    double S = e;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const double t = __shfl_up(S, 1 << j, 64);
      if (lane >= (1 << j)) S = fma(sc.pw[j], t, S);
    }
    if (lane == 63) wave_tot[wv] = S;
    __syncthreads();
    double O = 0.0;                                          // state entering this wave
    for (int u = 0; u < wv; u++) O = fma(sc.pw[6], O, wave_tot[u]);
    double st = __shfl_up(S, 1, 64);
    if (lane == 0) st = 0.0;
    st = fma(sc.apow[lane], O, st);                          // true state before this lane's first sample
    double w = st;
#pragma unroll
    for (int i = 0; i < FMR_DE_LPL; i++) {
      w = v[i] - a1 * w;
      mine[i] = b0 * w;
    }
  }
  __syncthreads();
  if (dbg) {
    double *dp = dbg + (long long)s * dbg_stride + dbg_off;
    for (int j = FMR_DE_WARMUP + tid; j < n_t; j += BLOCK) {
      const long long pos = r0 + j;
      if (pos >= 0 && pos < n_if) dp[pos] = de_xs[de_idx(j)];
    }
  }
  double *y = (ch ? y1 : y0) + (long long)s * y_stride + y_off;
  if constexpr (NA_T > 0) {
    constexpr int R = 4, SPAN = NA_T + (R - 1) * D_T;
    for (int q = tid; q * R < cnt; q += BLOCK) {
      const int r0 = q * R;
      const int jtop = FMR_DE_WARMUP + (NA_T - 1) + (r0 + R - 1) * D_T;     // newest sample of the run
      double acc[R] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int u = 0; u < SPAN; u++) {
        const double xv = de_xs[de_idx(jtop - u)];
#pragma unroll
        for (int i = 0; i < R; i++) {
          const int k = u - (R - 1 - i) * D_T;       // tap of output r0+i that meets this sample
          if (k >= 0 && k < NA_T) acc[i] = fir_step(hA[k], xv, acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < R; i++)
        if (r0 + i < cnt) y[m0 + r0 + i] = acc[i];
    }
  } else {
    for (int r = tid; r < cnt; r += BLOCK) {
      const int jt = FMR_DE_WARMUP + (NA - 1) + r * D;
      double acc = 0.0;
#pragma unroll 4
      for (int k = 0; k < NA; k++) acc = fir_step(hA[k], de_xs[de_idx(jt - k)], acc);
      y[m0 + r] = acc;
    }
  }
}

// ---------------------------------------------------------------------------
// DC block (HighPassFilterIir) by linear multiple shooting + output mux
// (FmDecode.cpp:194-220,242-283).
// ---------------------------------------------------------------------------
#define FMR_DC_K 32   // chunks per lane in the node pass
#define FMR_DC_MAXW 8  // waves per workgroup of the node pass (each lane keeps its 2 K chunk values in registers)
struct DcCoef {
  double b0, b1, b2, a1, a2;
  double ac[4];        // A^C row-major: state transition over one chunk
  double agp[6][4];    // (A^(C*K))^(2^k), k = 0..5: transitions over 1,2,4,..,32 lane groups
  double ac_lo[4], agp_lo[6][4];   // what the doubles above leave of the powers (make_dc_coef)
};

template <int C>
__global__ void k_dc_pass1(const double *__restrict__ p0, const double *__restrict__ p1, long long p_stride, int n,
                           DcCoef k, double *__restrict__ G, int nc, int ch_base) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y, ch = blockIdx.z + ch_base;
  if (c >= nc) return;
  const double *p = (ch ? p1 : p0) + (long long)s * p_stride;
  const int start = c * C, end = min(start + C, n);
  double x1 = 0.0, x2 = 0.0;
  serial_prefetch<8>(p, start, end, [&](int, double v) {
    const double x0 = v - (k.a1 * x1 + k.a2 * x2);
    x2 = x1; x1 = x0;
  });
  double *g = G + (((long long)s * 2 + ch) * nc + c) * 2;
  g[0] = x1; g[1] = x2;
}

// node pass: start[c+1] = G[c] + A^C start[c].  One wave per (stream, channel); every lane
// owns K consecutive chunks: it folds them into one vector q (K short steps), a log-step
// wave scan with the precomputed powers of A^(C K) turns the q's into the lane start
// states, and every lane replays its K chunks writing the chunk starts.  2048 chunks per
// pass, the pass end state carries into the next pass.
__device__ __forceinline__ void mv2(const double *m, double x1, double x2, double &y1, double &y2) {
  y1 = m[0] * x1 + m[1] * x2;
  y2 = m[2] * x1 + m[3] * x2;
}
// M x for a transition M = hi + lo over n samples.  M's entries are of size n r^n and the state's two words nearly equal: the
// two products of a row cancel, and rounded one by one they leave n ulp of the state in a chunk's start state, which the audio
// shows (its second difference).  Here a row's sum is rounded once: h1 x2 = p + e exactly, fma(h0, x1, p) the rounded sum.
__device__ __forceinline__ double mv2c_row(double h0, double h1, double l0, double l1, double x1, double x2) {
  const double p = h1 * x2, e = fma(h1, x2, -p);
  return (fma(h0, x1, p) + e) + (l0 * x1 + l1 * x2);
}
__device__ __forceinline__ void mv2c(const double *h, const double *l, double x1, double x2, double &y1, double &y2) {
  y1 = mv2c_row(h[0], h[1], l[0], l[1], x1, x2);
  y2 = mv2c_row(h[2], h[3], l[2], l[3], x1, x2);
}
__global__ __launch_bounds__(64 * FMR_DC_MAXW) void k_dc_nodes(const double *__restrict__ G, double *__restrict__ start, int nc,
                                                    DcCoef k, StreamState *st, int n_streams, int nch) {
  // blockDim.x = 64 * NW: the NW waves take consecutive 64*K-chunk segments of a pass, scan them with a zero
  // carry in parallel, chain the NW segment totals (A^(C K 64) per segment) and replay with the true carries.
  __shared__ double tot[16][2];
  __shared__ double endst[2];
  const int t = blockIdx.x;
  const int s = nch ? t / nch : t, ch = nch ? t % nch : 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, NW = blockDim.x >> 6;
  if (s >= n_streams) return;
  const double *g = G + (((long long)s * 2 + ch) * nc) * 2;
  double *o = start + (((long long)s * 2 + ch) * nc) * 2;
  double c1 = ch ? st[s].dc_st_x1 : st[s].dc_mono_x1;     // carry: state at the start of the pass
  double c2 = ch ? st[s].dc_st_x2 : st[s].dc_mono_x2;
  if (nch == 0) { c1 = st[s].am_dc_x1; c2 = st[s].am_dc_x2; }   // AmDecoder's DC block (one channel, its own state)
  constexpr int K = FMR_DC_K;
  // AG^64 = (AG^32)^2: transition over one wave segment (FM: 2^17 samples, entries of 1e-20 -- plain products do)
  double ag64[4];
  {
    const double *x = k.agp[5];
    ag64[0] = x[0] * x[0] + x[1] * x[2]; ag64[1] = x[0] * x[1] + x[1] * x[3];
    ag64[2] = x[2] * x[0] + x[3] * x[2]; ag64[3] = x[2] * x[1] + x[3] * x[3];
  }
  for (int c0 = 0; c0 < nc; c0 += 64 * K * NW) {
    const int cb = c0 + (wv * 64 + lane) * K;
    // my K chunks' end vectors into registers, all loads in flight at once (clamped, not predicated): fetched one by one
    // inside the fold and again inside the replay they were 2 K dependent memory latencies, 87 % of this kernel's time
    double g1[K], g2[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const double2 gv = *reinterpret_cast<const double2 *>(g + 2 * (long long)min(cb + j, nc - 1));
      g1[j] = gv.x; g2[j] = gv.y;
    }
    // fold my K chunks from zero state
    double q1 = 0.0, q2 = 0.0;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int c = cb + j;
      if (c < nc) {
        double n1, n2;
        mv2c(k.ac, k.ac_lo, q1, q2, n1, n2);
        q1 = n1 + g1[j]; q2 = n2 + g2[j];
      }
      // past the end: identity step would need A^-C; lanes past nc are never read back
    }
    // inclusive scan inside the wave: q_l <- sum_{i<=l} AG^(l-i) q_i
#pragma unroll
    for (int lv = 0; lv < 6; lv++) {
      const int o_ = 1 << lv;
      const double p1 = __shfl_up(q1, o_, 64), p2 = __shfl_up(q2, o_, 64);
      if (lane >= o_) {
        double m1, m2;
        mv2c(k.agp[lv], k.agp_lo[lv], p1, p2, m1, m2);
        q1 += m1; q2 += m2;
      }
    }
    if (lane == 63) { tot[wv][0] = q1; tot[wv][1] = q2; }
    __syncthreads();
    // carry entering my wave's segment (segments before a partial one are always full)
    double w1 = c1, w2 = c2;
    for (int u = 0; u < wv; u++) {
      double m1, m2;
      mv2(ag64, w1, w2, m1, m2);
      w1 = m1 + tot[u][0]; w2 = m2 + tot[u][1];
    }
    // my start = AG^lane * carry + (inclusive result of lane-1)
    double e1 = __shfl_up(q1, 1, 64), e2 = __shfl_up(q2, 1, 64);
    if (lane == 0) { e1 = 0.0; e2 = 0.0; }
    double t1 = w1, t2 = w2;
#pragma unroll
    for (int lv = 0; lv < 6; lv++) {
      if (lane & (1 << lv)) { double m1, m2; mv2c(k.agp[lv], k.agp_lo[lv], t1, t2, m1, m2); t1 = m1; t2 = m2; }
    }
    double x1 = t1 + e1, x2 = t2 + e2;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int c = cb + j;
      if (c < nc) {
        *reinterpret_cast<double2 *>(o + 2 * (long long)c) = make_double2(x1, x2);
        double n1, n2;
        mv2c(k.ac, k.ac_lo, x1, x2, n1, n2);
        x1 = n1 + g1[j]; x2 = n2 + g2[j];
      }
    }
    // carry into the next pass = state after the last chunk of the last lane (only used when the pass was full)
    if (wv == NW - 1 && lane == 63) { endst[0] = x1; endst[1] = x2; }
    __syncthreads();
    c1 = endst[0]; c2 = endst[1];
    __syncthreads();
  }
}

template <int C>
__global__ void k_dc_pass2_mux(const double *__restrict__ p0, const double *__restrict__ p1, long long p_stride,
                               BlockTab bt, int n, DcCoef k, const double *__restrict__ start, int nc, int stereo,
                               int pilot_shift, const int *__restrict__ stereo_blk, double *__restrict__ audio,
                               long long audio_stride, StreamState *st) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  if (c >= nc) return;
  const double *m = p0 + (long long)s * p_stride;
  const double *d = p1 + (long long)s * p_stride;
  double *out = audio + (long long)s * audio_stride;
  const int i0 = c * C, i1 = min(i0 + C, n);
  const double *sm = start + (((long long)s * 2 + 0) * nc + c) * 2;
  const double *sd = start + (((long long)s * 2 + 1) * nc + c) * 2;
  double m1 = sm[0], m2 = sm[1], d1 = 0.0, d2 = 0.0;
  if (stereo) { d1 = sd[0]; d2 = sd[1]; }
  // audio block that holds sample i0
  int b = 0;
  if (stereo) {
    int lo = 0, hi = bt.nb - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (bt.au_off[mid] <= i0) lo = mid; else hi = mid - 1;
    }
    b = lo;
    while (b < bt.nb - 1 && bt.au_len[b] == 0) b++;
  }
  int bend = stereo ? bt.au_off[b] + bt.au_len[b] : n;
  int locked = stereo ? stereo_blk[(long long)s * bt.nb + b] : 0;
  serial_prefetch2<8>(m, stereo ? d : m, i0, i1, [&](int i, double mv, double dv) {
    double x0 = mv - (k.a1 * m1 + k.a2 * m2);
    const double mm = k.b0 * x0 + k.b1 * m1 + k.b2 * m2;
    m2 = m1; m1 = x0;
    if (!stereo) { out[i] = mm; return; }
    x0 = dv - (k.a1 * d1 + k.a2 * d2);
    const double dd = k.b0 * x0 + k.b1 * d1 + k.b2 * d2;
    d2 = d1; d1 = x0;
    while (i >= bend && b < bt.nb - 1) {
      b++;
      bend = bt.au_off[b] + bt.au_len[b];
      locked = stereo_blk[(long long)s * bt.nb + b];
    }
    double l, r;
    if (locked) {
      if (pilot_shift) { l = r = dd; }
      else { const double ss = 1.017 * dd; l = mm + ss; r = mm - ss; }
    } else {
      if (pilot_shift) { l = r = 0.0; } else { l = r = mm; }
    }
    out[2 * i] = l; out[2 * i + 1] = r;
  });
  if (c == nc - 1) {
    st[s].dc_mono_x1 = m1; st[s].dc_mono_x2 = m2;
    if (stereo) { st[s].dc_st_x1 = d1; st[s].dc_st_x2 = d2; }
  }
}

// ---------------------------------------------------------------------------
// IF AGC by Newton multiple shooting.  nodes[c] = gain at the start of chunk c.
// ---------------------------------------------------------------------------
// Input of the AGC recurrence: the IF samples, or -- FM without the equaliser behind the fused front end, where the gain is
// solved for its carried state only and nobody else reads the IF -- |x|^2 as the front end's epilogue stored it (4 instead
// of 8 bytes per IF sample through HBM, both ways).  (g x)^2 + (g y)^2 against g^2 (x^2 + y^2): a few float ulps of the
// squared magnitude, 1e-11 of the gain's factor z -- far inside the dead zone the reference's own gain wanders in.
__device__ __forceinline__ float agc_nrm(float2 v, float g) { const float xr = v.x * g, xi = v.y * g; return xr * xr + xi * xi; }
__device__ __forceinline__ float agc_nrm(float e, float g) { return (g * g) * e; }
// node pass: v[c+1] = G[c] + M[c] (v[c] - old[c]); affine scan: every lane composes 8
// consecutive chunk maps serially, one wave scan covers 512 chunks, then every lane
// replays its 8 maps from its scanned start value.
#define FMR_AGC_PER_LANE 8
// (G and M are read with agent-scope loads: in k_agc_round they were stored by other workgroups of the same launch)
__device__ __forceinline__ void agc_node_pass(const int s, float *__restrict__ nodes, const float *G, const double *M,
                                              int nc, StreamState *st, IterFlags *fl, int gain_invariant) {
  // blockDim.x = 64 * NW: the NW waves take consecutive 64*K-chunk segments of a pass, scan their maps with an
  // identity carry in parallel, chain the NW segment maps and replay with the true carries (as k_dc_nodes).
  __shared__ double segA[16], segB[16];
  __shared__ double pass_end;
  __shared__ float wmax[16], wcut[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, NW = blockDim.x >> 6;
  float cut = 0.f;
  float *nd = nodes + (long long)s * (nc + 1);
  const float *g = G + (long long)s * nc;
  const double *m = M + (long long)s * nc;
  constexpr int K = FMR_AGC_PER_LANE;
  double carry = (double)nd[0];   // v[0] is the carried state, fixed
  float maxrel = 0.f;
  __shared__ float old_next;      // the node a tile's last lane overwrites is the OLD start of the next tile's first chunk
  // the next tile's maps are fetched while this tile is scanned (the pass was ten memory round trips in a row)
  double a_n[K];
  float g_n[K], o_n[K + 1];
  auto fetch = [&](int c0) {
    const int cb = c0 + (wv * 64 + lane) * K;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int c = cb + j;
      if (c < nc) {
        a_n[j] = __longlong_as_double(__hip_atomic_load((const long long *)&m[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        g_n[j] = __hip_atomic_load(&g[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else { a_n[j] = 1.0; g_n[j] = 0.f; }
    }
#pragma unroll
    for (int j = 0; j <= K; j++) o_n[j] = nd[min(cb + j, nc)];
  };
  fetch(0);
  for (int c0 = 0; c0 < nc; c0 += 64 * K * NW) {
    const int cb = c0 + (wv * 64 + lane) * K;
    double a[K], b[K];
    float oldn[K];
    // maps of this lane: v' = a v + b with b = G - a*old
    if (c0 > 0 && threadIdx.x == 0) o_n[0] = old_next;
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (cb + j < nc) { a[j] = a_n[j]; b[j] = (double)g_n[j] - a[j] * (double)o_n[j]; oldn[j] = o_n[j + 1]; }
      else { a[j] = 1.0; b[j] = 0.0; oldn[j] = 0.f; }
    }
    if (c0 + 64 * K * NW < nc) fetch(c0 + 64 * K * NW);
    double ca = 1.0, cbv = 0.0;               // composition of the lane's K maps
#pragma unroll
    for (int j = 0; j < K; j++) { cbv = a[j] * cbv + b[j]; ca = a[j] * ca; }
    // inclusive wave scan of the lane maps
    double sa = ca, sb = cbv;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double pa = __shfl_up(sa, o, 64), pb = __shfl_up(sb, o, 64);
      if (lane >= o) { sb = sa * pb + sb; sa = sa * pa; }
    }
    if (lane == 63) { segA[wv] = sa; segB[wv] = sb; }
    __syncthreads();                          // segment maps published; all old values of the pass are in registers
    double cw = carry;                        // carry entering my wave's segment
    for (int u = 0; u < wv; u++) cw = segA[u] * cw + segB[u];
    // exclusive value = start of this lane's first chunk
    double ea = __shfl_up(sa, 1, 64), eb = __shfl_up(sb, 1, 64);
    if (lane == 0) { ea = 1.0; eb = 0.0; }
    double v = ea * cw + eb;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int c = cb + j;
      v = a[j] * v + b[j];
      float vf = (float)v;
      if (c < nc) {
        // the linearisation can overflow a float (a cold call on silence: the gain grows by 1 + rate per sample and the
        // product of the chunk slopes over a thousand chunks is not finite), and 0 * inf behind a chunk that ended on the
        // clamp is a NaN that fmaxf below would not see -- a round was accepted with such nodes, their chunks' first gains
        // were not finite and the AM tail's DC block kept the NaN for good.  The chunk's own end value stands for such a
        // node (read again: this is the rare path), and the round is not accepted.
        if (!isfinite(vf)) { vf = __hip_atomic_load(&g[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); v = (double)vf; maxrel = INFINITY; }
        nd[c + 1] = vf;
        maxrel = fmaxf(maxrel, fabsf(vf - oldn[j]) / fmaxf(fabsf(vf), 1e-30f));
        if (a[j] == 0.0) cut = 1.f;          // the chunk ran into the gain clamp or the non-finite reset (k_agc_round: dg = 0)
      }
    }
    if (wv == NW - 1 && lane == 63) {
      const double pe = (double)(float)(sa * cw + sb);
      pass_end = isfinite(pe) ? pe : (double)(float)v;      // (a full tile: this lane's v is the node the next tile starts from)
      old_next = oldn[K - 1];
    }
    __syncthreads();
    carry = pass_end;
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { maxrel = fmaxf(maxrel, __shfl_xor(maxrel, o, 64)); cut = fmaxf(cut, __shfl_xor(cut, o, 64)); }
  if (lane == 0) { wmax[wv] = maxrel; wcut[wv] = cut; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int u = 1; u < NW; u++) { maxrel = fmaxf(maxrel, wmax[u]); cut = fmaxf(cut, wcut[u]); }
  if (threadIdx.x != 0) return;
  {
    if (fl[s].agc_iters < 16) fl[s].agc_hist[fl[s].agc_iters] = maxrel;
    fl[s].agc_iters++;
    fl[s].agc_resid = maxrel;
    // Two regimes.  Amplitude-modulated input (AM): z moves by many ulps per sample,
    // the map is smooth and Newton reaches <= 1e-6 in 2-4 rounds.  Constant-envelope
    // input (FM): |r (1 - |x g|^2)| < ulp(1)/2 most of the time, so z == 1.0f exactly
    // and the reference's gain only random-walks inside a dead zone ~3e-4 wide; there
    // the chunk map has no usable slope and the rounds stagnate at a few 1e-5.  That
    // is also the level at which the reference's own gain depends on FMA contraction
    // (hazard H7), and atan2 is invariant to it: accept <= 5e-5 from round 2 on -- only where the consumer
    // is invariant to the gain (FM discriminator).  AM audio scales with the gain: there the rounds go on until
    // no node moves by more than one float ulp.
    // Over thousands of nodes a float node somewhere keeps flipping its last bit, so "one ulp everywhere" is not
    // reachable on long calls: from round 3 on a movement of 5e-6 is accepted as well (below).
    // gain_invariant == 2: nobody reads the per-sample gains of this call either (FM without the equaliser, no debug tap)
    // -- the call is solved for the carried state only, and the node pass has just computed that state from the first
    // integration pass: a second pass would only rewrite gains that are never read.  Round 1 is accepted at the same 5e-5.
    // ... and when only the state is wanted, round 1 is accepted up to a movement of 2e-3 as well: the node pass has just
    // applied the first-order correction to every node, what it leaves is second order -- 1.3 x movement^2 in a float64
    // model of this recurrence over noise levels 1e-3 ... 1e-1 (tools/agc_round_model.py: movement 1.0e-3 -> error 8.5e-7,
    // 5.3e-3 -> 3.2e-5, 1.1e-2 -> 1.6e-4), so <= 5e-6 here, a tenth of what the later rounds are accepted at and below the
    // 3e-5 they stagnate at.  A second round could only measure that: it was 0.08-0.1 ms of the side stream for every call
    // of a noisy input (sigma 1e-2: movement 2.8e-4) or behind the IF filter (5.8e-5).  The model is of the smooth recurrence:
    // a call in which some chunk ran into the gain clamp or the non-finite reset (the discontinuous branches, dg = 0) takes
    // its second round.
    // Round 6, measured on calls of 2048 blocks (tools/am_tol_check.py, AM 384 kS/s -> 48 k): the node movements of such a call
    // run 3.5e-3, 6e-6, 2e-6, 1.2e-6, 7e-7 -- from the third round on a factor two per round against the float dead zone --
    // and the audio's RMS distance from the oracle is 7e-8 when the fifth round is the accepted one (movement <= 1e-6, rounds
    // 1-5), 1.1e-7 ... 2.2e-7 with the third (<= 5e-6, now) and 4.5e-7 ... 9.2e-7 with the second: two rounds of 0.073 ms
    // bought a factor two at 1 % of the 1e-5 tolerance.
    // (gain_invariant < 0, diagnostic builds: -n = the AM acceptance in units of 1e-6, from round 3 on; -1000 - n: from round 2 on)
    const float tight = gain_invariant > 0 ? 1.0e-6f : 1.5e-7f;
    const int am_r0 = gain_invariant <= -1000 ? 2 : 3;
    const float am_tol = gain_invariant < 0 ? 1.0e-6f * (float)((-gain_invariant) % 1000) : 5.0e-6f;
    if (maxrel <= tight || (gain_invariant > 0 && (fl[s].agc_iters >= 2 || gain_invariant == 2) && maxrel <= 5.0e-5f) ||
        (gain_invariant == 2 && fl[s].agc_iters == 1 && maxrel <= 2.0e-3f && cut == 0.f) ||
        (gain_invariant <= 0 && fl[s].agc_iters >= am_r0 && maxrel <= am_tol)) {   // gains of the last shoot pass stand
      // The gains in HBM are those of the pass BEFORE this node pass: they are off by the movement just measured.  Where the
      // audio scales with them (AM family) that is up to 5e-6, and the audio AGC behind ends the call that far from the
      // reference's (1.3e-6 of af_agc_gain on a steady USB call of 2056 chunks accepted at 3e-6; the tolerance is 1e-6).  The
      // next launch then runs its integration pass from the nodes just written and no node pass (agc_converged == 2 -> 1):
      // what it leaves is the next movement, a third of this one (2.6e-6 -> 7.8e-7 in a float restatement of these rounds,
      // af_agc_gain 1.3e-6 -> 2.5e-7).  A movement of 5e-7 or less needs none, and the last round has no launch behind it.
      fl[s].agc_converged = (gain_invariant <= 0 && maxrel > 5.0e-7f) ? 2 : 1;
      st[s].agc_gain = nd[nc];
    }
  }
}
// One Newton round in one launch: the integration pass, a chunk per lane; the workgroup of a stream that finishes last runs
// the node pass (last-arrival ticket, as the PLL's rounds: nobody waits for anybody).  Launched with FOUR waves per
// workgroup: the node pass of the two-launch form was one workgroup of sixteen, which finds no compute unit with room for
// all its waves while the PLL's first pass holds the chip (0.1 ms of waiting per round, measured: 1024 threads 0.125 ms per
// round, 256 threads 0.087, 64 threads -- a one-wave node pass -- 0.166).
template <int C, class XT>
__global__ __launch_bounds__(256) void k_agc_round(const XT *__restrict__ x, long long x_stride, int x_off, int n,
                                                    float *__restrict__ gain, long long g_stride, float *__restrict__ nodes,
                                                    float *G, double *M, int nc, float initial_gain, float max_gain,
                                                    float rate, StreamState *st, IterFlags *fl, int gain_invariant,
                                                    unsigned int *__restrict__ ticket) {
  __shared__ int s_last;
  const int s = blockIdx.y;
  // (stable for the whole launch: the node pass that sets it runs after every workgroup of the stream has passed here)
  const int conv = fl[s].agc_converged;       // 0: the rounds go on; 2: accepted, one more integration pass for its gains; 1: done
  if (conv == 1) return;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nc) {
    const XT *xs = x + (long long)s * x_stride + x_off;
    float *gs = gain ? gain + (long long)s * g_stride : nullptr;
    const int i0 = c * C, i1 = min(i0 + C, n);
    float g = nodes[(long long)s * (nc + 1) + c];
    double dg = 1.0;
    const double r = (double)rate;
    serial_prefetch<8>(xs, i0, i1, [&](int i, XT v) {
      if (gs) gs[i] = g;
      const float nrm = agc_nrm(v, g);
      const float z = (float)(1.0 + (r * (1.0 - (double)nrm)));
      const float gn = g * z;
      // d(g z)/dg = z + g dz/dg = z - 2 r nrm   (nrm ~ g^2)
      dg *= ((double)z - 2.0 * r * (double)nrm);
      g = gn;
      if (!isfinite(g)) { g = initial_gain; dg = 0.0; }
      else if (g > max_gain) { g = max_gain; dg = 0.0; }
    });
    __hip_atomic_store(&G[(long long)s * nc + c], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((long long *)&M[(long long)s * nc + c], __double_as_longlong(dg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       // this wave's stores are acknowledged by the L2
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = __hip_atomic_fetch_add(&ticket[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (t == gridDim.x - 1);
    if (s_last) __hip_atomic_store(&ticket[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!s_last) return;
  if (conv == 2) { if (threadIdx.x == 0) fl[s].agc_converged = 1; return; }
  agc_node_pass(s, nodes, G, M, nc, st, fl, gain_invariant);
}

__global__ void k_iter_begin(IterFlags *fl, float *__restrict__ agc_nodes, int agc_nc, const StreamState *st,
                             int n_streams, unsigned long long *__restrict__ pll_sync, int sync_words,
                             unsigned int *__restrict__ pll_tick2, int n_tick2, unsigned int *__restrict__ agc_tick) {
  const int s = blockIdx.x;
  if (s >= n_streams) return;
  if (threadIdx.x == 0) {
    fl[s] = IterFlags{};
    if (agc_tick) agc_tick[s] = 0u;        // k_agc_round's last-arrival ticket: left at zero by a launch that completes, not by one that was aborted
    if (agc_nodes) agc_nodes[(long long)s * (agc_nc + 1)] = st[s].agc_gain;
  }
  // the PLL rounds' tickets and maximum slots (PllSync) are left at zero by the kernels that use them; a call that
  // starts from anything else (an aborted call before it) would mistake its last arrivals, so they are zeroed anyway
  if (pll_sync) {
    for (int i = threadIdx.x; i < sync_words; i += blockDim.x) pll_sync[(long long)s * sync_words + i] = 0ull;
    for (int i = threadIdx.x; i < n_tick2; i += blockDim.x) pll_tick2[(long long)s * n_tick2 + i] = 0u;
  }
  // initial guess: the carried gain everywhere
  if (agc_nodes) {
    const float g0 = st[s].agc_gain;
    for (int c = 1 + threadIdx.x; c <= agc_nc; c += blockDim.x) agc_nodes[(long long)s * (agc_nc + 1) + c] = g0;
  }
}

// serial fallback wrapper: only when the iteration did not converge
template <class XT>
__global__ void k_if_agc_fallback(const XT *__restrict__ x, long long x_stride, int x_off, int n,
                                  float *__restrict__ gain, long long g_stride, StreamState *st, int n_streams,
                                  float initial_gain, float max_gain, float rate, IterFlags *fl) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams || fl[s].agc_converged) return;
  fl[s].agc_fallback = 1;
  const XT *xs = x + (long long)s * x_stride + x_off;
  float *gs = gain ? gain + (long long)s * g_stride : nullptr;
  float g = st[s].agc_gain;
  const double r = (double)rate;
  for (int i = 0; i < n; i++) {
    const XT v = xs[i];
    if (gs) gs[i] = g;
    const float nrm = agc_nrm(v, g);
    const float z = (float)(1.0 + (r * (1.0 - (double)nrm)));
    g *= z;
    if (!isfinite(g)) g = initial_gain;
    else if (g > max_gain) g = max_gain;
  }
  st[s].agc_gain = g;
}

// ---------------------------------------------------------------------------
// AmDecoder audio tail in time-parallel form (AmDecode.cpp:190-216): DC block -> AfSimpleAgc -> de-emphasis.
//  * DC block: linear multiple shooting (k_dc_pass1 / k_dc_nodes above give every chunk its start state);
//  * AfSimpleAgc (AfSimpleAgc.cpp:36-56): Newton multiple shooting on the gain, as the IF AGC -- every chunk is
//    integrated with the reference's arithmetic from its node value together with d g_end / d g_start, the node pass
//    solves the linearised boundary conditions; the DC block is re-run inside the shoot kernel (6 flops per sample),
//    so no intermediate signal is stored; the gain clamp (1.5) makes most chunks end ON the clamp: zero sensitivity;
//  * de-emphasis (tau = 4.8 samples): every chunk warms up over FMR_AM_DE_WARM samples (e^{-160/4.8} = 3e-15).
// If the Newton rounds do not converge the serial kernel (k_am_tail) runs instead.
// ---------------------------------------------------------------------------
#define FMR_AM_DE_WARM 160
struct AfAgcCoef { double init, maxg, ref, rate; };

__device__ __forceinline__ void af_node_pass(int s, double *__restrict__ nodes, const double *G, const double *M, int nc,
                                             StreamState *st, IterFlags *fl);
// One Newton round in one launch (round 6; k_af_shoot + k_af_nodes before: twelve launches of ~9 us for the six rounds of a
// call): the integration pass, a chunk per lane, one wave per workgroup; the workgroup of a stream that finishes last runs
// the node pass (last-arrival ticket, as k_agc_round).
template <int C>
__global__ __launch_bounds__(64) void k_af_round(const double *__restrict__ demod, long long d_stride, int n, DcCoef k,
                           const double *__restrict__ dc_start, AfAgcCoef af, double *__restrict__ nodes,
                           double *G, double *M, double *__restrict__ agc_out, long long o_stride,
                           int nc, StreamState *st, IterFlags *fl, unsigned int *__restrict__ ticket) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  // (stable for the whole launch: the node pass that sets it runs after every workgroup of the stream has passed here)
  if (fl[s].af_converged) return;
  if (c < nc) {
  const double *x = demod + (long long)s * d_stride;
  double *o = agc_out + (long long)s * o_stride;
  const int i0 = c * C, i1 = min(i0 + C, n);
  const double *sd = dc_start + (((long long)s * 2) * nc + c) * 2;
  double x1 = sd[0], x2 = sd[1];
  double g = nodes[(long long)s * (nc + 1) + c], dg = 1.0;
  serial_prefetch<8>(x, i0, i1, [&](int i, double xv) {
    const double x0 = xv - (k.a1 * x1 + k.a2 * x2);                 // Filter.cpp:243-250 (DF2)
    const double v = k.b0 * x0 + k.b1 * x1 + k.b2 * x2;
    x2 = x1; x1 = x0;
    const double xg = v * g;                                         // AfSimpleAgc.cpp:41-47
    o[i] = xg * af.ref;
    const double sq = xg * xg;
    const double z = 1.0 + (af.rate * (1.0 - sq));
    dg *= (z - 2.0 * af.rate * sq);                                  // d(g z)/dg, sq ~ g^2
    g *= z;
    if (!isfinite(g)) { g = af.init; dg = 0.0; }
    else if (g > af.maxg) { g = af.maxg; dg = 0.0; }
  });
  __hip_atomic_store((long long *)&G[(long long)s * nc + c], __double_as_longlong(g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store((long long *)&M[(long long)s * nc + c], __double_as_longlong(dg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (c == nc - 1) { st[s].am_dc_x1_next = x1; st[s].am_dc_x2_next = x2; }   // DC-block state after the call (exact: linear pass)
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       // this wave's stores are acknowledged by the L2
  int last = 0;
  if (threadIdx.x == 0) {
    const unsigned int t = __hip_atomic_fetch_add(&ticket[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == gridDim.x - 1);
    if (last) __hip_atomic_store(&ticket[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  last = __builtin_amdgcn_readfirstlane(last);
  if (!last) return;
  af_node_pass(s, nodes, G, M, nc, st, fl);
}

// node pass of the AF AGC: v[c+1] = G[c] + M[c] (v[c] - old[c]); one wave per stream, K chunk maps per lane.
// (G and M are read with agent-scope loads: in k_af_round they were stored by other workgroups of the same launch)
__device__ __forceinline__ void af_node_pass(int s, double *__restrict__ nodes, const double *G, const double *M, int nc,
                                             StreamState *st, IterFlags *fl) {
  const int lane = threadIdx.x;
  double *nd = nodes + (long long)s * (nc + 1);
  const double *g = G + (long long)s * nc, *m = M + (long long)s * nc;
  auto ld = [](const double *p) { return __longlong_as_double(__hip_atomic_load((const long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); };
  constexpr int K = 8;
  double carry = nd[0], maxrel = 0.0;
  double old_next = 0.0;          // the node a tile's last lane overwrites is the OLD start of the next tile's first chunk (as agc_node_pass)
  for (int c0 = 0; c0 < nc; c0 += 64 * K) {
    const int cb = c0 + lane * K;
    double a[K], b[K], oldn[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int c = cb + j;
      if (c < nc) {
        const double o = (j == 0 && lane == 0 && c0 > 0) ? old_next : nd[c];
        a[j] = ld(m + c); b[j] = ld(g + c) - a[j] * o; oldn[j] = nd[c + 1];
      }
      else { a[j] = 1.0; b[j] = 0.0; oldn[j] = 0.0; }
    }
    old_next = readlane_d(oldn[K - 1], 63);
    double ca = 1.0, cbv = 0.0;
#pragma unroll
    for (int j = 0; j < K; j++) { cbv = a[j] * cbv + b[j]; ca = a[j] * ca; }
    double sa = ca, sb = cbv;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double pa = __shfl_up(sa, o, 64), pb = __shfl_up(sb, o, 64);
      if (lane >= o) { sb = sa * pb + sb; sa = sa * pa; }
    }
    double ea = __shfl_up(sa, 1, 64), eb = __shfl_up(sb, 1, 64);
    if (lane == 0) { ea = 1.0; eb = 0.0; }
    double v = ea * carry + eb;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int c = cb + j;
      v = a[j] * v + b[j];
      if (c < nc) {
        // the linearisation can overflow (a cold start on a weak signal: the product of M > 1 over hundreds of chunks), and
        // 0 * inf behind a chunk that ended on the clamp is a NaN that fmax below would not see: the chunk's own end
        // value stands for such a node (read again: this is the rare path) and the round is not accepted
        if (!isfinite(v)) { v = ld(g + c); maxrel = INFINITY; }
        nd[c + 1] = v; maxrel = fmax(maxrel, fabs(v - oldn[j]) / fmax(fabs(v), 1e-300));
      }
    }
    const double cn = readlane_d(sa, 63) * carry + readlane_d(sb, 63);
    carry = isfinite(cn) ? cn : readlane_d(v, 63);      // (a full tile: lane 63's v is the node the next tile starts from)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) maxrel = fmax(maxrel, __shfl_xor(maxrel, o, 64));
  if (lane != 0) return;
  fl[s].af_iters++;
  fl[s].af_resid = maxrel;
  // the trajectory of the last shoot pass stands once no node moves by more than 1e-13 relative; where the gain keeps
  // touching its clamp inside chunks the map is only piecewise smooth and the last digits wander: 1e-9 from round 4 on
  // (1e-9 of the audio, four orders inside the tolerance)
  if (maxrel <= 1e-13 || (fl[s].af_iters >= 4 && maxrel <= 1e-9)) {
    fl[s].af_converged = 1;
    st[s].af_gain = nd[nc];
  }
}

__global__ void k_af_begin(IterFlags *fl, double *__restrict__ nodes, int nc, const StreamState *st, unsigned int *__restrict__ ticket) {
  const int s = blockIdx.x;
  if (threadIdx.x == 0) { fl[s].af_converged = 0; fl[s].af_iters = 0; fl[s].af_fallback = 0; fl[s].af_resid = 0.0; ticket[s] = 0u; }
  const double g0 = st[s].af_gain;
  for (int c = threadIdx.x; c <= nc; c += blockDim.x) nodes[(long long)s * (nc + 1) + c] = g0;
}

// de-emphasis + output (AmDecode.cpp:212-217); do_deemph = 0: copy (DSB / SSB / CW modes have none)
template <int C>
__global__ void k_am_deemph_out(const double *__restrict__ agc_out, long long o_stride, int n, double b0, double a1,
                                int do_deemph, double *__restrict__ audio, long long audio_stride, StreamState *st,
                                const IterFlags *__restrict__ fl) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = blockIdx.y;
  const int nc = (n + C - 1) / C;
  if (c >= nc || !fl[s].af_converged) return;
  const double *x = agc_out + (long long)s * o_stride;
  double *out = audio + (long long)s * audio_stride;
  const int i0 = c * C, i1 = min(i0 + C, n);
  if (!do_deemph) { for (int i = i0; i < i1; i++) out[i] = x[i]; return; }
  double e1;
  int w0 = i0 - FMR_AM_DE_WARM;
  if (w0 <= 0) { w0 = 0; e1 = st[s].am_de_x1; } else e1 = 0.0;     // the first chunks run from the carried state
  for (int i = w0; i < i0; i++) e1 = x[i] - a1 * e1;
  serial_prefetch<8>(x, i0, i1, [&](int i, double v) {
    const double w = v - a1 * e1;
    out[i] = b0 * w;
    e1 = w;
  });
  if (c == nc - 1) {
    // commit after every chunk that reads the carried state has done so: those are the first ceil(WARM / C) + 1 chunks,
    // and they run in the first workgroup of the launch while this is the last lane of the last one -- unless the call
    // is that short, in which case the state is staged and committed by k_am_commit
    st[s].am_de_x1_next = e1;
  }
}
__global__ void k_am_commit(StreamState *st, IterFlags *fl, int n_streams) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  if (fl[s].af_converged) { st[s].am_de_x1 = st[s].am_de_x1_next; st[s].am_dc_x1 = st[s].am_dc_x1_next; st[s].am_dc_x2 = st[s].am_dc_x2_next; }
}

// ---------------------------------------------------------------------------
// Pilot PLL by Newton multiple shooting.
// State vector: 0 phase, 1 freq, 2 loop-filter delay (previous phase error),
// 3,4 biquad-I delays, 5,6 biquad-Q delays.
// ---------------------------------------------------------------------------
struct PllRegs { double v[7]; double li, lq, freq_err; double sn, cs; };   // li,lq: biquad outputs of the last sample; sn,cs: sin / cos of v[0]
__device__ __forceinline__ double pll_level(const PllRegs &S) { return sqrt((S.li * S.li) + (S.lq * S.lq)); }  // PilotPhaseLock.cpp:106

struct ChunkTab {
  const int *off;   // [nck] IF-sample offset of the chunk inside the call
  const int *len;   // [nck]
  const int *blk;   // [nck] block it belongs to
  const int *first; // [nb+1] first chunk of each block
  int nck;
};

// End-of-decoder mark for the pipelined chain: a counter in pinned host memory the caller polls.
__global__ void k_signal_host(unsigned long long *flag, unsigned long long value) {
  __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Per-call block table: pinned host slot -> device slot (the host pointer is device-visible).
// two ranges in one launch (the pipelined chain's front-end tables: a launch on the critical stream costs microseconds)
__global__ void k_copy_ints2(const int *__restrict__ src0, int *__restrict__ dst0, int n0, const int *__restrict__ src1,
                             int *__restrict__ dst1, int n1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n0) dst0[i] = src0[i];
  else if (i - n0 < n1) dst1[i - n0] = src1[i - n0];
}

__global__ void k_copy_ints(const int *__restrict__ src, int *__restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = __builtin_nontemporal_load(src + i);
}

// Chunk table from the block table: block b owns chunks first[b] .. first[b+1]-1, each c_pll
// IF samples (the last one shorter).  One wave per block.
__global__ __launch_bounds__(64) void k_chunk_tab(const int *__restrict__ if_off, const int *__restrict__ if_len,
                                                  const int *__restrict__ first, int c_pll, int *__restrict__ ck_off,
                                                  int *__restrict__ ck_len, int *__restrict__ ck_blk) {
  const int b = blockIdx.x;
  const int f = first[b], n = first[b + 1] - f, off = if_off[b], len = if_len[b];
  for (int j = threadIdx.x; j < n; j += 64) {
    ck_off[f + j] = off + j * c_pll;
    ck_len[f + j] = min(c_pll, len - j * c_pll);
    ck_blk[f + j] = b;
  }
}

__device__ __forceinline__ double wrap_pm_pi(double d) {
  const double two_pi = 2.0 * 3.14159265358979323846;
  if (d > 3.14159265358979323846) d -= two_pi;
  if (d < -3.14159265358979323846) d += two_pi;
  return d;
}

// sin and cos of the PLL phase (PilotPhaseLock.cpp:78-79 calls std::sin / std::cos).  The phase lives in
// (0, 2 pi + maxfreq], so the general-range machinery of the library sincos (about 100 of the ~200 instructions
// of a sample step, all on the loop-carried chain) is not needed: two-constant Cody-Waite reduction by pi/2
// (exact for |n| < 2^20) and the classic degree-13/14 minimax kernels on [-pi/4, pi/4].  Absolute error
// <= 2.3e-16 (checked against a correctly rounded reference over the whole range), i.e. the same last-bit class as
// the difference between two libm implementations.
__device__ __forceinline__ void pll_sincos(double x, double &sn, double &cs) {
  const double n = rint(x * 6.36619772367581382433e-01);            // 2/pi
  double r = fma(-n, 1.57079632673412561417e+00, x);                // pi/2, first 33 bits
  r = fma(-n, 6.07710050650619224932e-11, r);                       // pi/2 - the above
  const double z = r * r;
  double ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = fma(z, ps, 2.75573137070700676789e-06);
  ps = fma(z, ps, -1.98412698298579493134e-04);
  ps = fma(z, ps, 8.33333333332248946124e-03);
  ps = fma(z, ps, -1.66666666666666324348e-01);
  const double sp = fma(r * z, ps, r);
  double pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = fma(z, pc, -2.75573143513906633035e-07);
  pc = fma(z, pc, 2.48015872894767294178e-05);
  pc = fma(z, pc, -1.38888888888741095749e-03);
  pc = fma(z, pc, 4.16666666666666019037e-02);
  const double cp = fma(z * z, pc, fma(z, -0.5, 1.0));
  const int q = (int)n & 3;
  const double a = (q & 1) ? cp : sp, b = (q & 1) ? sp : cp;
  sn = (q & 2) ? -a : a;
  cs = ((q + 1) & 2) ? -b : b;
}

// sin / cos of the NEXT phase from the current pair: turned by the phase increment f of the sample.  A lone wave issues an
// instruction every ~4.8 cycles whatever it is, and pll_sincos is 60 of the 150 instructions of a sample step; the phase
// increment lives in [minfreq, maxfreq], 2 pi 30 / 384000 = 4.9e-4 either side of the middle f0 of the range, where its sine
// and cosine are fourth-order polynomials (the fifth-order term is 2e-19): eight fused multiply-adds, four operations for
// the rotation.  The pair is set from pll_sincos at the head of every chunk (64 samples), so it is never more than 64
// rotations -- 1e-14 -- away from it.  (Explicit fma: this is not reference arithmetic, like pll_sincos itself.)
struct PllRot { double f0, S0, C0, nS0, s2, s3, s4, c2, c3, c4; };
__device__ __forceinline__ PllRot pll_rot_make(const PllConst &pc) {
  PllRot r;
  r.f0 = 0.5 * (pc.minfreq + pc.maxfreq);
  pll_sincos(r.f0, r.S0, r.C0);
  r.nS0 = -r.S0;
  r.s2 = -0.5 * r.S0; r.s3 = -r.C0 / 6.0; r.s4 = r.S0 / 24.0;
  r.c2 = -0.5 * r.C0; r.c3 = r.S0 / 6.0; r.c4 = r.C0 / 24.0;
  // (held in registers: the compiler would recompute the derived ones per sample)
  asm volatile("" : "+v"(r.s2), "+v"(r.c2), "+v"(r.nS0));
  return r;
}
__device__ __forceinline__ void pll_rotate(double &sn, double &cs, double f, const PllRot &r) {
  const double d = f - r.f0;
  const double sd = fma(d, fma(d, fma(d, fma(d, r.s4, r.s3), r.s2), r.C0), r.S0);
  const double cd = fma(d, fma(d, fma(d, fma(d, r.c4, r.c3), r.c2), r.nS0), r.C0);
  const double ns = fma(cs, sd, sn * cd), nc = fma(-sn, sd, cs * cd);
  sn = ns; cs = nc;
}

// One PLL sample step, the reference's arithmetic (PilotPhaseLock.cpp:73-151);
// JAC: also advance the 7x7 sensitivity Mx = d state / d start-state.
template <bool JAC>
__device__ __forceinline__ int pll_step(PllRegs &S, double x, const PllConst &pc, const PllRot &rot, const float *tab, int pilot_shift,
                                        double &out, double (*Mx)[7]) {
  const double two_pi = 2.0 * 3.14159265358979323846;
  const double psin = S.sn, pcos = S.cs;        // (PilotPhaseLock.cpp:78-79: sin / cos of the phase, carried along -- pll_rotate)
  const double carrier = pilot_shift ? (2 * pcos * pcos - 1) : (2 * psin * pcos);
  out = (carrier * x) * 2.0;
  const double phasor_i = psin * x, phasor_q = pcos * x;
  const double wi0 = phasor_i - (pc.bq_a1 * S.v[3] + pc.bq_a2 * S.v[4]);
  const double wq0 = phasor_q - (pc.bq_a1 * S.v[5] + pc.bq_a2 * S.v[6]);
  const double new_i = pc.bq_b0 * wi0, new_q = pc.bq_b0 * wq0;
  const double e = (double)fast_atan2f_dev((float)new_q, (float)new_i, tab);
  S.li = new_i; S.lq = new_q;   // m_pilot_level = sqrt(i*i + q*q) is only consumed after a block's last sample
  const double y = pc.lf_b0 * e + pc.lf_b1 * S.v[2];
  S.freq_err = y;
  const double f_un = S.v[1] + y;
  // fmax(minfreq, fmin(maxfreq, f_un)) (:96-97) without the two canonicalising v_max the compiler puts in front of a
  // constant operand it cannot prove quiet (same two instructions, same result: they return the other operand for a NaN)
  double f_new;
  asm("v_min_f64 %0, %1, %2" : "=v"(f_new) : "v"(f_un), "s"(pc.maxfreq));
  asm("v_max_f64 %0, %1, %2" : "=v"(f_new) : "v"(f_new), "s"(pc.minfreq));
  pll_rotate(S.sn, S.cs, f_new, rot);
  if (JAC) {
    const double den = wi0 * wi0 + wq0 * wq0;
    // (one reciprocal -- v_rcp_f64 and a Newton step -- instead of two fp64 divisions of ~20 instructions each: the
    // sensitivities are this implementation's own quantity and steer a chord iteration, they need no last bit)
    double inv = __builtin_amdgcn_rcp(den);
    inv = fma(fma(-den, inv, 1.0), inv, inv);
    const double eI = den > 0.0 ? -wq0 * inv : 0.0, eQ = den > 0.0 ? wi0 * inv : 0.0;
    const double cI = x * pcos, cQ = -x * psin;
    const double mask = (f_un >= pc.minfreq && f_un <= pc.maxfreq) ? 1.0 : 0.0;
    const double na1 = -pc.bq_a1, na2 = -pc.bq_a2;
#pragma unroll
    for (int k = 0; k < 7; k++) {
      // (explicit fma: the sensitivities are this implementation's own quantity, not reference arithmetic)
      const double rwi = fma(cI, Mx[0][k], fma(na1, Mx[3][k], na2 * Mx[4][k]));
      const double rwq = fma(cQ, Mx[0][k], fma(na1, Mx[5][k], na2 * Mx[6][k]));
      const double re = fma(eI, rwi, eQ * rwq);
      const double rf = mask * fma(pc.lf_b0, re, fma(pc.lf_b1, Mx[2][k], Mx[1][k]));
      Mx[0][k] = Mx[0][k] + rf;
      Mx[1][k] = rf;
      Mx[2][k] = re;
      Mx[4][k] = Mx[3][k];
      Mx[3][k] = rwi;
      Mx[6][k] = Mx[5][k];
      Mx[5][k] = rwq;
    }
  }
  S.v[2] = e;
  S.v[4] = S.v[3]; S.v[3] = wi0;
  S.v[6] = S.v[5]; S.v[5] = wq0;
  S.v[1] = f_new;
  double ph = S.v[0] + f_new;
  int wrapped = 0;
  if (ph > two_pi) { ph -= two_pi; wrapped = 1; }
  S.v[0] = ph;
  return wrapped;
}

// Round bookkeeping shared by the three-launch form of the Newton round (described at k_pll_up below)
struct PllSync {
  unsigned int tick_shoot, tick_up;
  unsigned long long rslot[64];       // integration pass: scaled boundary mismatch maxima (bits of non-negative doubles)
  unsigned long long dslot[64][8];    // node pass: scaled Newton step maxima per state component
};

// true for exactly one workgroup (of one wave) of a set of `total`: the one that arrives last.  No cache-wide fence:
// a release / acquire pair at agent scope writes back and invalidates the whole L2 of the XCD on this part -- once per
// workgroup that made every kernel on the GPU slower (measured: PLL group 0.33 -> 0.54 ms, k_stats beside it 0.18 ->
// 0.31 ms).  Instead everything one workgroup hands to another inside a launch is stored and loaded with agent-scope
// atomic accesses (write-through / L2-coherent), the producer waits for its stores to be acknowledged before it takes
// its ticket, and the ticket itself is an agent-scope atomic.  The ticket is left at zero for the next launch.
// This is NOT the HIP / LLVM memory model's release-acquire: it relies on gfx950's write-through agent-scope stores and
// on s_waitcnt vmcnt(0) meaning "acknowledged by the L2".  Hence (i) the guard below, (ii) the rule that everything
// handed over inside a launch goes through st_agent / ld_agent / atomics -- the buffers written with PLAIN stores in
// these kernels (the `pre` composites and `ds` start deltas of k_pll_up, the nodes of k_pll_down, IterFlags by the
// last arrival) are only read by LATER launches -- and (iii) tests/test_gpu_pll_forms.py: the three-launch form against
// the seven-launch form (FMR_PLL_V1, no in-launch hand-off) over many rounds and streams: identical decisions, audio to 1e-9.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the in-launch hand-off of the PLL rounds is validated on gfx950 only"
#endif
__device__ __forceinline__ void st_agent(double *p, double v) {
  __hip_atomic_store((long long *)p, __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_agent(const double *p) {
  return __longlong_as_double(__hip_atomic_load((const long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ bool pll_last_arrival(unsigned int *ticket, unsigned int total) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");       // this workgroup's stores and atomics are done
  unsigned int t = 0;
  if (threadIdx.x == 0) t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  t = (unsigned int)__builtin_amdgcn_readfirstlane((int)t);
  if (t != total - 1) return false;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::: "memory");
  return true;
}
__device__ __forceinline__ unsigned long long pll_max_bits(double v) {   // fmax semantics: a NaN never wins
  return (v > 0.0) ? (unsigned long long)__double_as_longlong(v) : 0ull;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// k_pll_check's bookkeeping on one wave: same acceptance rule, same record in IterFlags
__device__ __forceinline__ void pll_round_check(IterFlags &F, PllSync &Y, double tol, double rtol, int have_d,
                                                bool may_accept) {
  const int lane = threadIdx.x;
  const double mr = wave_max_d(__longlong_as_double((long long)__hip_atomic_load(&Y.rslot[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
  __hip_atomic_store(&Y.rslot[lane], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (reset for the next launch: atomic like every other access to the slots)
  double mc[7];
#pragma unroll
  for (int q = 0; q < 7; q++) {
    mc[q] = wave_max_d(__longlong_as_double((long long)__hip_atomic_load(&Y.dslot[lane][q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    __hip_atomic_store(&Y.dslot[lane][q], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane != 0) return;
  double m = 0.0;
#pragma unroll
  for (int q = 0; q < 7; q++) { m = fmax(m, mc[q]); if (have_d) F.pll_comp[q] = mc[q]; }
  const int it = F.pll_iters;                    // integration passes done before this one
  if (it < 16) F.pll_rhist[it] = mr;
  if (have_d && it >= 1 && it <= 16) F.pll_hist[it - 1] = m;
  F.pll_iters = it + 1;
  if (may_accept && mr <= rtol) { F.pll_converged = 1; F.pll_r_accepted = 1; F.pll_resid = mr; }
  else if (may_accept && have_d && m <= tol) { F.pll_converged = 1; F.pll_resid = m; }
  else F.pll_resid = have_d ? m : mr;
}

#define FMR_NODE_GRP 32    // chunks per level-1 group of the node pass (below)
#define FMR_NODE_GRP2 32   // level-1 groups per level-2 group
// The up-sweep of the node pass from a group's Jacobians and mismatches in LDS (defined with the node pass below): the
// integration pass that has just computed them runs it in its own tail (round 5), k_pll_up stages them from HBM first.
// TE: the composites of the tree's inner nodes' earlier halves (pll_compose_tree's sink), FMR_TREE_SINK maps per group: the
// tail of the Jacobian pass leaves them, the head of the pass behind it descends through them (pll_descend_tree).
struct PllUpArgs { double *PQ, *PRE, *PQ2; int ngrp, ngrp2; double *dstart2; PllSync *sync; unsigned int *tick2; double *TE; };
// ... and the down-sweep of the node pass in the HEAD of the pass that integrates from its result (pll_down_group).
// TE != null: as a descent through the Jacobian pass's tree (the pass right behind it); null: the chain (chord rounds, whose
// mismatches are no longer the ones the stored composites were made from).
struct PllDownArgs { const double *PRE, *dstart2; int ngrp, ngrp2; double minfreq, maxfreq; const double *wave_first; const double *TE; };
__device__ __forceinline__ void pll_down_group(const PllDownArgs &dn, double *nodes_s, const double *g, const double *m, int nck, int s, int grp,
                                               PllSync *sync, double *sm, double *sr, double *so, double *first, int lane);
__device__ __forceinline__ void pll_descend_head(const PllDownArgs &dn, double *nd, const double *g, const double *m, int nck, int s,
                                                 PllSync *sync, double *xs, int lane, double (&sv)[7], double (&nxt)[7]);
__device__ __forceinline__ void pll_up_from_lds(const PllUpArgs &u, int s, int grp, int n, double *sm, double *sh, int lane);
__device__ __forceinline__ void pll_up_levels23(const PllUpArgs &u, int s, int grp, double val, double *sm, double *sh, int lane);
__device__ __forceinline__ void pll_stage_group(const double *__restrict__ m, const double *__restrict__ g, const double *__restrict__ nd,
                                                int c0, int n, int lane, double *sm, double *sr, double *so, int rs = 8);

// WOUT: store the demodulated L-R samples and the wrap masks.  The first round's trajectory is never the accepted one
// (its start nodes are the nominal ramp), so it skips the 8 bytes per sample.
//
// One lane integrates one chunk, so lane l's sample i sits c_pll doubles away from lane l+1's: read or written straight
// from the loop, every wave instruction touches 64 cache lines.  Measured (round 2, SQ / TA counters): the second pass
// spent 14 us per SIMD in its VALU and the rest of its 80 us waiting for the acknowledgement of such stores (gfx9 has one
// in-order counter for loads and stores, so the wait for the next samples is a wait for the last stores).  Samples
// therefore cross between HBM and the lanes through an LDS tile: the wave loads T samples of each of its 64 chunks
// with row-contiguous instructions (half a wave per chunk), every lane then walks its own row, the results overwrite
// the inputs in place, and the tile leaves the same way.  No global access inside the sample loop.
template <bool JAC, bool WOUT>
__global__ __launch_bounds__(64) void k_pll_shoot(const fm_mpx_t *__restrict__ base, long long base_stride, int base_off, ChunkTab ct,
                            double *__restrict__ raw, long long raw_stride, int raw_off,
                            const float *__restrict__ atan_tab, PllConst pc, int pilot_shift,
                            const double *__restrict__ nodes, double *__restrict__ G, double *__restrict__ M,
                            int *__restrict__ ck_wraps, unsigned long long *__restrict__ ck_mask, int mask_words,
                            IterFlags *__restrict__ fl, double *__restrict__ wg_r,
                            PllSync *__restrict__ sync, double tol, double rtol, int have_d,
                            PllUpArgs up = PllUpArgs{} /* JAC pass, PQ != null: the node pass's up-sweep runs in this launch's tail */,
                            PllDownArgs dn = PllDownArgs{} /* PRE != null: ... and its down-sweep in this launch's head (nodes is then written) */,
                            double *__restrict__ wave_first = nullptr /* [S][workgroups][7]: the start node of every wave's first chunk, for the next down-sweep */) {
  constexpr int T = 32, TP = T + 1;          // tile: 64 rows of T samples, one pad word pair per row
#ifdef FMR_PLL_TRACE   // diagnostic build: where and when every workgroup ran (tools/pll_trace.py reads the dump)
  const unsigned long long trace_t0 = __builtin_readcyclecounter(), trace_w0 = wall_clock64();
#endif
  __shared__ float tab[257];
  __shared__ __attribute__((aligned(16))) double xs[64 * TP];
  __shared__ int s_off[64], s_len[64];
  static_assert(64 * TP >= FMR_NODE_GRP * FMR_MAP, "the tile also carries a group's maps [M | r] out and into the up-sweep's tree");
  static_assert(64 * TP >= FMR_NODE_GRP2 * 56 + 64, "... and stages levels 2 and 3 of the up-sweep");
  static_assert(FMR_NODE_GRP <= FMR_TREE_MAXN && FMR_MAP == 56, "pll_compose_tree's sizes");
  // the integration passes are the decoder stream's critical kernels and share their SIMDs with the audio tail of the call
  // before: their waves win the issue arbitration (round 6: 0.4742 -> 0.4711 ms per step over four interleaved 100-step
  // runs each; without the tail stage the step is 0.4465)
  __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x;
  const int c = blockIdx.x * blockDim.x + lane;
  const int s = blockIdx.y;
  const bool valid = c < ct.nck;
  const int cc = valid ? c : ct.nck - 1;
  // Everything the head reads from memory -- the stream's flag, the chunk's length and offset, its start node and the
  // atan table -- is in flight together and waited for once: behind the test of the flag the same loads were a second
  // dependent round trip at the head of every pass.  Same addresses as before, whatever the flag says.
  const int done = fl[s].pll_converged;
  float tabv[5];
#pragma unroll
  for (int u = 0; u < 5; u++) tabv[u] = atan_tab[min(lane + 64 * u, 256)];
  const int len_c = ct.len[cc];
  const int off = ct.off[cc];
  const double *nd = nodes + ((long long)s * (ct.nck + 1) + cc) * 7;
  const bool nodes_from_sweep = !JAC && dn.PRE != nullptr;      // (the down-sweep below writes `nodes`: not read here then)
  double nd0[7];
#pragma unroll
  for (int k = 0; k < 7; k++) nd0[k] = nodes_from_sweep ? 0.0 : nd[k];
  // (the compiler would otherwise sink the loads behind the branch, next to their first use)
  asm volatile("" ::"v"(tabv[0]), "v"(tabv[1]), "v"(tabv[2]), "v"(tabv[3]), "v"(tabv[4]), "v"(len_c), "v"(off), "v"(nd0[0]),
               "v"(nd0[1]), "v"(nd0[2]), "v"(nd0[3]), "v"(nd0[4]), "v"(nd0[5]), "v"(nd0[6]));
  if (done) return;                         // uniform: every workgroup of the stream leaves
#pragma unroll
  for (int u = 0; u < 5; u++) if (lane + 64 * u < 257) tab[lane + 64 * u] = tabv[u];
  const int n = valid ? len_c : 0;
  s_off[lane] = off; s_len[lane] = n;
  int nmax = n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
  const fm_mpx_t *xb = base + (long long)s * base_stride + base_off;
  double *ob = raw + (long long)s * raw_stride + raw_off;
  double rmax = 0.0;
  PllRegs S;
  double nxt[7];                             // start node of the NEXT chunk (the boundary mismatch at the end)
  if (!JAC && dn.PRE && dn.TE) {
    // ---- the node pass's down-sweep behind a Jacobian round: a descent through that round's tree (pll_descend_head)
    pll_descend_head(dn, const_cast<double *>(nodes) + (long long)s * (ct.nck + 1) * 7, G + (long long)s * ct.nck * 9,
                     M + (long long)s * ct.nck * 49, ct.nck, s, sync, xs, lane, S.v, nxt);
  } else if (!JAC && dn.PRE) {
    // ---- the node pass's down-sweep for this wave's two groups of 32 chunks, here: k_pll_down was a launch of its own
    // (26 us + a launch gap) whose every workgroup did 32 dependent 7 x 7 steps and went away.  A wave needs the new start
    // nodes of ITS chunks only: those of chunks c0 + 1 .. from its own two sweeps, that of its first chunk from the group's
    // prefix composite (pll_down_group) -- nothing another wave of this launch writes.
    double *sm = xs, *sr = xs + FMR_NODE_GRP * 49, *so = sr + FMR_NODE_GRP * 7, *first = so + FMR_NODE_GRP * 7;
    static_assert(64 * TP >= FMR_NODE_GRP * (49 + 7 + 7) + 8, "down-sweep staging");
    double *nds = const_cast<double *>(nodes) + (long long)s * (ct.nck + 1) * 7;
    const double *gb = G + (long long)s * ct.nck * 9;
    const double *mb2 = M + (long long)s * ct.nck * 49;
#pragma unroll
    for (int k = 0; k < 7; k++) { S.v[k] = 0.0; nxt[k] = 0.0; }
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
      const int grp = 2 * blockIdx.x + h, c0 = grp * FMR_NODE_GRP;
      if (c0 >= ct.nck) break;
      __syncthreads();
      pll_down_group(dn, nds, gb, mb2, ct.nck, s, grp, sync, sm, sr, so, first, lane);
      __syncthreads();
      // lane l of this half starts chunk c0 + t (t = l & 31): t = 0 from `first` (h = 0) / the other half's last node
      // (h = 1, kept in `carry`), t >= 1 from so[t - 1]; its next node is so[t]
      const int t = lane & 31;
      if ((lane >> 5) == h) {
#pragma unroll
        for (int k = 0; k < 7; k++) {
          if (t > 0) S.v[k] = so[(t - 1) * 7 + k];
          else if (h == 0) S.v[k] = first[k];
          nxt[k] = so[t * 7 + k];
        }
      }
      if (h == 0) {      // chunk c0 + 32's start node = the last node of this sweep: lane 32 takes it
#pragma unroll
        for (int k = 0; k < 7; k++) if (lane == 32) S.v[k] = so[31 * 7 + k];
      }
    }
    __syncthreads();
  } else {
#pragma unroll
    for (int k = 0; k < 7; k++) { S.v[k] = nd0[k]; nxt[k] = 0.0; }
  }
  const bool nxt_in_regs = !JAC && dn.PRE != nullptr;       // (else the next chunk's start node is read where it is needed)
  if (wave_first && lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; k++) wave_first[((long long)s * gridDim.x + blockIdx.x) * 7 + k] = S.v[k];
  }
  S.li = 0.0; S.lq = 0.0; S.freq_err = 0.0;
  pll_sincos(S.v[0], S.sn, S.cs);
  const PllRot rot = pll_rot_make(pc);
  double Mx[7][7];
#pragma unroll
  for (int r = 0; r < 7; r++)
#pragma unroll
    for (int k = 0; k < 7; k++) Mx[r][k] = (r == k) ? 1.0 : 0.0;
  int wraps = 0;
  // positions of the phase wraps inside the chunk (bit i = sample i wrapped): lets the
  // finish pass place a PPS event without re-integrating the chunk
  unsigned long long *mk = ck_mask + ((long long)s * ct.nck + cc) * mask_words;
  unsigned long long word = 0;
  const int half = lane >> 5, l5 = lane & 31;
  for (int t0 = 0; t0 < nmax; t0 += T) {
    __syncthreads();
    // tile in: lanes 0-31 take chunk j, lanes 32-63 chunk j+1 (clamped addresses instead of predicates: loads under a
    // branch make the compiler wait for each of them)
    // (all loads of a tile in flight at once: one memory latency per tile.  The Jacobian variant took them eight at a time
    // while it needed 226 registers without them; since the rotation and the reciprocal it has room: 246 with all 32)
    constexpr int NLD = 32;
#pragma unroll 1
    for (int j0 = 0; j0 < 64; j0 += 2 * NLD) {
      double v[NLD];
#pragma unroll
      for (int u = 0; u < NLD; u++) {
        const int jj = j0 + 2 * u + half;
        const int o0 = s_off[jj], last = o0 + s_len[jj] - 1;
        v[u] = (double)xb[max(0, min(o0 + t0 + l5, last))];
      }
#pragma unroll
      for (int u = 0; u < NLD; u++) xs[(j0 + 2 * u + half) * TP + l5] = v[u];
    }
    __syncthreads();
    const int m = min(T, n - t0);
    double *row = xs + lane * TP;
    // (two samples per pass: the delay-line moves of the state and of the sensitivities become register names)
    auto sample = [&](int i) {
      double o;
      const int wflag = pll_step<JAC>(S, row[i], pc, rot, tab, pilot_shift, o, Mx);
      wraps += wflag;
      if (WOUT) {
        const int gi = t0 + i;
        word |= (unsigned long long)wflag << (gi & 63);
        if ((gi & 63) == 63) { mk[gi >> 6] = word; word = 0; }
        row[i] = o;
      }
    };
    int i = 0;
    for (; i + 2 <= m; i += 2) { sample(i); sample(i + 1); }
    if (i < m) sample(i);
    if (WOUT) {
      __syncthreads();
#pragma unroll 8
      for (int j = 0; j < 64; j += 2) {
        const int jj = j + half;
        if (l5 < s_len[jj] - t0) ob[s_off[jj] + t0 + l5] = xs[jj * TP + l5];
      }
    }
  }
  if (valid) {
    if (WOUT && (n & 63)) mk[n >> 6] = word;
    double *g = G + ((long long)s * ct.nck + c) * 9;
#pragma unroll
    for (int k = 0; k < 7; k++) g[k] = S.v[k];
    g[7] = pll_level(S); g[8] = S.freq_err;
    ck_wraps[(long long)s * ct.nck + c] = wraps;
    // scaled mismatch against the start node of the next chunk (same scales as the node pass);
    // the call's end node has no consumer
    if (c + 1 < ct.nck) {
      const double wsc = 1.0 / (1e-7 * (fabs(S.v[3]) + fabs(S.v[5]) + 1.0));
      auto nx = [&](int k) { return nxt_in_regs ? nxt[k] : nd[7 + k]; };
      rmax = fabs(wrap_pm_pi(S.v[0] - nx(0))) * 1e7;
      rmax = fmax(rmax, fabs(S.v[1] - nx(1)) * 1e9);
      rmax = fmax(rmax, fabs(S.v[2] - nx(2)) * 1e5);
#pragma unroll
      for (int k = 3; k < 7; k++) rmax = fmax(rmax, fabs(S.v[k] - nx(k)) * wsc);
    }
  }
  if (JAC) {   // JAC == false: frozen-Jacobian round, the stored M of the last JAC round stands
    // Every lane holds its chunk's Jacobian and boundary mismatch.  A group of 32 chunks at a time, the lanes put their
    // maps [M | r] into the tile (7 rows of 8), and from there
    //  - the Jacobians leave for HBM (the down-sweep and the chord rounds read them): the group's are one contiguous block
    //    of 32 x 49 doubles, so a store instruction covers one or two rows instead of 64 (row-per-lane stores are
    //    issue-bound in the TA);
    //  - the node pass's up-sweep composes the group's maps, here: k_pll_up would start behind a launch boundary, with every
    //    workgroup of this pass gone, and read the 31 MB of Jacobians of a 2^27-sample call back from HBM.  The maps come
    //    from the registers, not from the stores (no wait for them, no way back through L2), and are composed pairwise in
    //    five levels, four pairs a round on 56 lanes with four independent entries each (pll_compose_tree: nine rounds a
    //    group; the chain of k_pll_up is 32 dependent steps of one entry per lane).  Same maps, bit for bit, as k_pll_up
    //    stages; another association.
    double *mb = M + ((long long)s * ct.nck + (long long)blockIdx.x * 64) * 49;
    double rr[7];
#pragma unroll
    for (int k = 0; k < 7; k++) rr[k] = S.v[k] - nd[7 + k];          // pll_mismatch of this chunk
    rr[0] = wrap_pm_pi(rr[0]);
    double pq0 = 0.0, pq1 = 0.0;      // the two groups' composites, one entry per lane
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
      const int grp = 2 * blockIdx.x + h, c0 = grp * FMR_NODE_GRP;
      if (c0 >= ct.nck) break;
      const int ng = min(FMR_NODE_GRP, ct.nck - c0);
      __syncthreads();
      if (half == h) {
        double *mp = xs + l5 * FMR_MAP;
#pragma unroll
        for (int r = 0; r < 7; r++) {
#pragma unroll
          for (int k = 0; k < 7; k++) mp[r * 8 + k] = Mx[r][k];
          mp[r * 8 + 7] = rr[r];
        }
      }
      __syncthreads();
      double *mg = mb + h * (FMR_NODE_GRP * 49);
#pragma unroll 5
      for (int it = 0; it < (FMR_NODE_GRP * 49 + 63) / 64; it++) {
        const int q = it * 64 + lane, r = q / 49, e = q - r * 49, er = e / 7;
        if (q < ng * 49) mg[q] = xs[r * FMR_MAP + er * 8 + (e - er * 7)];
      }
      if (up.PQ) {
        pll_compose_tree<64>(xs, ng, lane, [] { __syncthreads(); },
                             up.TE ? up.TE + ((long long)s * up.ngrp + grp) * (FMR_TREE_SINK * FMR_MAP) : nullptr);
        const double val = lane < FMR_MAP ? xs[lane] : 0.0;        // lane i * 8 + k: P[i][k], k == 7: q[i]
        if (h == 0) pq0 = val; else pq1 = val;
      }
    }
    // levels 2 and 3 behind both trees: they stage a set's maps through registers, which the Jacobians still held
    // above (in between the pass needs more than 256 registers: one wave per SIMD)
#pragma unroll 1
    for (int h = 0; h < 2 && up.PQ; h++) {
      const int grp = 2 * blockIdx.x + h;
      if (grp * FMR_NODE_GRP >= ct.nck) break;
      __syncthreads();
      pll_up_levels23(up, s, grp, h ? pq1 : pq0, xs, xs + FMR_NODE_GRP2 * 56, lane);
    }
  }
#ifdef FMR_PLL_TRACE
  if (threadIdx.x == 0 && (JAC || WOUT)) {
    unsigned int hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    unsigned long long *tr = (unsigned long long *)wg_r + (((long long)s * gridDim.x + blockIdx.x) * 2 + (JAC ? 0 : 1)) * 4;
    tr[0] = trace_w0; tr[1] = __builtin_readcyclecounter() - trace_t0; tr[2] = ((unsigned long long)xcc << 32) | hw;
    tr[3] = wall_clock64();
  }
#endif
  // per-workgroup maximum; k_pll_check (next launch) reduces them and may accept the round on the
  // mismatch alone, which skips this round's node pass
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, o, 64));
  if (!sync) {                               // seven-kernel form: k_pll_check is the next launch
    if (threadIdx.x == 0) wg_r[(long long)s * gridDim.x + blockIdx.x] = rmax;
    return;
  }
  // three-kernel form: maxima through 64 slots; the stream's last workgroup does the round's bookkeeping
  PllSync &Y = sync[s];
  if (threadIdx.x == 0) atomicMax(&Y.rslot[blockIdx.x & 63], pll_max_bits(rmax));
  if (pll_last_arrival(&Y.tick_shoot, gridDim.x)) pll_round_check(fl[s], Y, tol, rtol, have_d, WOUT);
}

// ---------------------------------------------------------------------------
// Node pass as a three-phase parallel scan of 7-dimensional affine maps.
// With d[c] = new[c] - old[c] and the boundary mismatch r[c] = G[c] - old[c+1]
// (phase component wrapped), the Newton update is the linear recurrence
//     d[c+1] = M[c] d[c] + r[c],   d[0] = 0.
//   A: every group of FMR_NODE_GRP chunks composes its maps into one (P | q)   (parallel)
//   B: one wave walks the group maps: start delta of every group               (short serial)
//   C: every group propagates its deltas, updates the nodes, records residuals  (parallel)
// Convergence scales: the phase error e is a FLOAT (fast_atan2f), so the chunk map has
// rounding discontinuities of one float ulp of e (<= 2.4e-7 while the loop acquires,
// ~1e-9 in lock), i.e. ~7e-11 in freq per flip; scales sit above that floor:
// phase 1e-7 rad, freq 1e-9, phase error 1e-5, biquad delays 1e-7 of the (I,Q) pair.
// ---------------------------------------------------------------------------
// mismatch r[c][i] = G[c][i] - old[c+1][i]
__device__ __forceinline__ double pll_mismatch(const double *g, const double *nd, int c, int i) {
  double v = g[(long long)c * 9 + i] - nd[(long long)(c + 1) * 7 + i];
  if (i == 0) v = wrap_pm_pi(v);
  return v;
}

// Phase A: lane (i*8 + k): k < 7 -> P[i][k], k == 7 -> q[i].  [P|q] <- [M P | M q + r].
// The group's 32 Jacobians are one contiguous 12.5 KB block: the wave stages it (and the mismatches) into LDS with
// coalesced loads issued all at once, then runs the dependent chain out of LDS.  (Round 1 fetched row by row, four
// chunks ahead: 288 eight-byte gather instructions per group and one memory latency per batch -- 59 us per pass.)
__device__ __forceinline__ void pll_stage_group(const double *__restrict__ m, const double *__restrict__ g,
                                                const double *__restrict__ nd, int c0, int n, int lane,
                                                double *sm, double *sr, double *so, int rs /* row stride of sr / so */) {
  constexpr int NL = (FMR_NODE_GRP * 49 + 63) / 64;
  const double *mb = m + (long long)c0 * 49;
  double tmp[NL];
#pragma unroll
  for (int u = 0; u < NL; u++) { const int idx = lane + 64 * u; tmp[u] = (idx < n * 49) ? mb[idx] : 0.0; }
  constexpr int NR = (FMR_NODE_GRP * 7 + 63) / 64;
  double tr[NR], to[NR];
#pragma unroll
  for (int u = 0; u < NR; u++) {
    const int idx = lane + 64 * u;
    const int c = idx / 7, q = idx - 7 * c;
    tr[u] = 0.0; to[u] = 0.0;
    if (idx < n * 7) {
      tr[u] = pll_mismatch(g, nd, c0 + c, q);
      if (so) to[u] = nd[(long long)(c0 + c + 1) * 7 + q];
    }
  }
#pragma unroll
  for (int u = 0; u < NL; u++) { const int idx = lane + 64 * u; if (idx < FMR_NODE_GRP * 49) sm[idx] = tmp[u]; }
#pragma unroll
  for (int u = 0; u < NR; u++) {
    const int idx = lane + 64 * u;
    const int c = idx / 7, q = idx - 7 * c;
    if (idx < FMR_NODE_GRP * 7) { sr[c * rs + q] = tr[u]; if (so) so[c * rs + q] = to[u]; }
  }
}

#ifdef FMR_AB_PARTNERS      // seven launches per Newton round (round 1): the partner tests/test_gpu_pll_forms.py compares the product with
__global__ __launch_bounds__(64) void k_pll_nodes_a(const double *__restrict__ nodes, const double *__restrict__ G,
                                                    const double *__restrict__ M, int nck,
                                                    double *__restrict__ PQ, const IterFlags *__restrict__ fl) {
  __shared__ double sm[FMR_NODE_GRP * 49];
  __shared__ double sr[FMR_NODE_GRP * 8];
  __shared__ double sh[64];
  const int s = blockIdx.y, grp = blockIdx.x;
  if (fl[s].pll_converged) return;
  const int lane = threadIdx.x, i = lane >> 3, k = lane & 7;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  const double *nd = nodes + (long long)s * (nck + 1) * 7;
  const double *g = G + (long long)s * nck * 9;
  const double *m = M + (long long)s * nck * 49;
  const int c0 = grp * FMR_NODE_GRP, c1 = min(c0 + FMR_NODE_GRP, nck);
  pll_stage_group(m, g, nd, c0, c1 - c0, lane, sm, sr, nullptr);
  __syncthreads();
  double val = (act && i == k) ? 1.0 : 0.0;   // P = I, q = 0
  for (int t = 0; t < c1 - c0; t++) {
    sh[lane] = val;
    __syncthreads();                      // one wave per block: just orders the LDS write
    double acc = (k == 7) ? sr[t * 8 + ii] : 0.0;
    const double *row = sm + t * 49 + ii * 7;
#pragma unroll
    for (int j = 0; j < 7; j++) acc = fma(row[j], sh[j * 8 + k], acc);
    __syncthreads();
    val = acc;
  }
  if (act) PQ[(((long long)s * gridDim.x + grp) * 7 + i) * 8 + k] = val;
}
#endif

// Phase A2: compose FMR_NODE_GRP2 consecutive level-1 group maps (already in [P|q] form)
// into one level-2 map; same lane layout as phase A.
// the [P|q] maps of one level-2 group (FMR_NODE_GRP2 x 56 doubles, contiguous) through LDS: one round of coalesced loads
template <bool AGENT = false>   // AGENT: the maps were stored by other workgroups of this launch (st_agent)
__device__ __forceinline__ void pll_stage_pq(const double *pq, int g0, int n, int lane, double *sp) {
  constexpr int NL = (FMR_NODE_GRP2 * 56 + 63) / 64;
  const double *pb = pq + (long long)g0 * 56;
  double tmp[NL];
#pragma unroll
  for (int u = 0; u < NL; u++) {
    const int idx = lane + 64 * u;
    tmp[u] = (idx < n * 56) ? (AGENT ? ld_agent(pb + idx) : pb[idx]) : 0.0;
  }
#pragma unroll
  for (int u = 0; u < NL; u++) { const int idx = lane + 64 * u; if (idx < FMR_NODE_GRP2 * 56) sp[idx] = tmp[u]; }
}

#ifdef FMR_AB_PARTNERS      // seven launches per Newton round (round 1): the partner tests/test_gpu_pll_forms.py compares the product with
__global__ __launch_bounds__(64) void k_pll_nodes_a2(const double *__restrict__ PQ1, int ngrp1,
                                                     double *__restrict__ PQ2, const IterFlags *__restrict__ fl) {
  __shared__ double sp[FMR_NODE_GRP2 * 56];
  __shared__ double sh[64];
  const int s = blockIdx.y, grp = blockIdx.x;
  if (fl[s].pll_converged) return;
  const int lane = threadIdx.x, i = lane >> 3, k = lane & 7;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  const double *pq = PQ1 + (long long)s * ngrp1 * 56;
  const int g0 = grp * FMR_NODE_GRP2, g1 = min(g0 + FMR_NODE_GRP2, ngrp1);
  pll_stage_pq(pq, g0, g1 - g0, lane, sp);
  __syncthreads();
  double val = (act && i == k) ? 1.0 : 0.0;
  for (int t = 0; t < g1 - g0; t++) {
    const double *mr = sp + (t * 7 + ii) * 8;
    sh[lane] = val;
    __syncthreads();
    double acc = (k == 7) ? mr[7] : 0.0;
#pragma unroll
    for (int j = 0; j < 7; j++) acc = fma(mr[j], sh[j * 8 + k], acc);
    __syncthreads();
    val = acc;
  }
  if (act) PQ2[(((long long)s * gridDim.x + grp) * 7 + i) * 8 + k] = val;
}
#endif

// Phase C2: from the start delta of a level-2 group, the start deltas of its level-1 groups
#ifdef FMR_AB_PARTNERS      // seven launches per Newton round (round 1): the partner tests/test_gpu_pll_forms.py compares the product with
__global__ __launch_bounds__(64) void k_pll_nodes_c2(const double *__restrict__ PQ1, int ngrp1,
                                                     const double *__restrict__ dstart2, double *__restrict__ dstart1,
                                                     const IterFlags *__restrict__ fl) {
  __shared__ double sp[FMR_NODE_GRP2 * 56];
  __shared__ double sd[FMR_NODE_GRP2 * 7];
  const int s = blockIdx.y, grp = blockIdx.x;
  if (fl[s].pll_converged) return;
  const int i = threadIdx.x;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  const double *pq = PQ1 + (long long)s * ngrp1 * 56;
  double *ds = dstart1 + (long long)s * ngrp1 * 7;
  const int g0 = grp * FMR_NODE_GRP2, g1 = min(g0 + FMR_NODE_GRP2, ngrp1);
  double d = dstart2[((long long)s * gridDim.x + grp) * 7 + ii];
  pll_stage_pq(pq, g0, g1 - g0, i, sp);
  __syncthreads();
  for (int t = 0; t < g1 - g0; t++) {
    if (act) sd[t * 7 + i] = d;
    const double *row = sp + (t * 7 + ii) * 8;
    const double d0 = readlane_d(d, 0), d1 = readlane_d(d, 1), d2 = readlane_d(d, 2), d3 = readlane_d(d, 3),
                 d4 = readlane_d(d, 4), d5 = readlane_d(d, 5), d6 = readlane_d(d, 6);
    const double p0 = fma(row[0], d0, fma(row[1], d1, row[7]));
    const double p1 = fma(row[2], d2, row[3] * d3);
    const double p2 = fma(row[4], d4, fma(row[5], d5, row[6] * d6));
    d = p0 + (p1 + p2);
  }
  __syncthreads();
  for (int idx = i; idx < (g1 - g0) * 7; idx += 64) ds[(long long)g0 * 7 + idx] = sd[idx];
}
#endif

// Phase B: delta at the start of every group (one wave per stream, lane i = component i);
// the rows of the group maps are fetched two batches ahead of the dependent chain.
struct PqRow { double v[8]; };
#ifdef FMR_AB_PARTNERS      // seven launches per Newton round (round 1): the partner tests/test_gpu_pll_forms.py compares the product with
__global__ __launch_bounds__(64) void k_pll_nodes_b(const double *__restrict__ PQ, int ngrp,
                                                    double *__restrict__ dstart, const IterFlags *__restrict__ fl) {
  const int s = blockIdx.x, i = threadIdx.x;
  if (fl[s].pll_converged) return;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  const double *pq = PQ + (long long)s * ngrp * 56;
  double *ds = dstart + (long long)s * ngrp * 7;
  double d = 0.0;
  constexpr int NB = 4;
  PqRow A[NB], B[NB];
  auto load = [&](int g0, PqRow *L) {
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int gq = min(g0 + j, ngrp - 1);
#pragma unroll
      for (int k = 0; k < 8; k++) L[j].v[k] = pq[((long long)gq * 7 + ii) * 8 + k];
    }
  };
  auto run = [&](int g0, const PqRow *L) {
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const int gq = g0 + j;
      if (gq >= ngrp) break;
      if (act) ds[(long long)gq * 7 + i] = d;
      const double d0 = readlane_d(d, 0), d1 = readlane_d(d, 1), d2 = readlane_d(d, 2), d3 = readlane_d(d, 3),
                   d4 = readlane_d(d, 4), d5 = readlane_d(d, 5), d6 = readlane_d(d, 6);
      const double p0 = fma(L[j].v[0], d0, fma(L[j].v[1], d1, L[j].v[7]));
      const double p1 = fma(L[j].v[2], d2, L[j].v[3] * d3);
      const double p2 = fma(L[j].v[4], d4, fma(L[j].v[5], d5, L[j].v[6] * d6));
      d = p0 + (p1 + p2);
    }
  };
  load(0, A);
  for (int g0 = 0; g0 < ngrp; g0 += 2 * NB) {
    load(g0 + NB, B);
    run(g0, A);
    load(g0 + 2 * NB, A);
    run(g0 + NB, B);
  }
}
#endif

// Phase C: propagate inside every group, update the nodes, record the scaled residual.  Jacobians, mismatches and
// old node values of the group are staged through LDS first (as in phase A; all old values are read before any node
// is rewritten: chunk c reads node c+1 and writes node c+1, a group only touches its own nodes); the new nodes leave
// through LDS too, as one coalesced block.
#ifdef FMR_AB_PARTNERS      // seven launches per Newton round (round 1): the partner tests/test_gpu_pll_forms.py compares the product with
__global__ __launch_bounds__(64) void k_pll_nodes_c(double *__restrict__ nodes, const double *__restrict__ G,
                                                    const double *__restrict__ M, int nck,
                                                    const double *__restrict__ dstart, IterFlags *fl,
                                                    double minfreq, double maxfreq, double *__restrict__ grp_resid) {
  __shared__ double sm[FMR_NODE_GRP * 49];
  __shared__ double sr[FMR_NODE_GRP * 8];
  __shared__ double so[FMR_NODE_GRP * 8];
  const int s = blockIdx.y, grp = blockIdx.x;
  if (fl[s].pll_converged) return;
  const int i = threadIdx.x;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  double *nd = nodes + (long long)s * (nck + 1) * 7;
  const double *g = G + (long long)s * nck * 9;
  const double *m = M + (long long)s * nck * 49;
  const double two_pi = 2.0 * 3.14159265358979323846, inv_two_pi = 1.0 / two_pi;
  const int c0 = grp * FMR_NODE_GRP, c1 = min(c0 + FMR_NODE_GRP, nck);
  double d = dstart[((long long)s * gridDim.x + grp) * 7 + ii];
  // scale of the biquad delays: size of the (I,Q) delay pair at the group start
  const double wm = fabs(g[(long long)c0 * 9 + 3]) + fabs(g[(long long)c0 * 9 + 5]);
  double inv_scale = 1.0 / (1e-7 * (wm + 1.0));
  if (i == 0) inv_scale = 1e7; else if (i == 1) inv_scale = 1e9; else if (i == 2) inv_scale = 1e5;
  pll_stage_group(m, g, nd, c0, c1 - c0, i, sm, sr, so);
  __syncthreads();
  double resid = 0.0;
  for (int t = 0; t < c1 - c0; t++) {
    const double *row = sm + t * 49 + ii * 7;
    const double d0 = readlane_d(d, 0), d1 = readlane_d(d, 1), d2 = readlane_d(d, 2), d3 = readlane_d(d, 3),
                 d4 = readlane_d(d, 4), d5 = readlane_d(d, 5), d6 = readlane_d(d, 6);
    const double p0 = fma(row[0], d0, fma(row[1], d1, sr[t * 8 + ii]));
    const double p1 = fma(row[2], d2, row[3] * d3);
    const double p2 = fma(row[4], d4, fma(row[5], d5, row[6] * d6));
    d = p0 + (p1 + p2);                       // delta of node c+1
    double nv = so[t * 8 + ii] + d;
    if (i == 0) {                             // keep the phase inside (0, 2 pi] like the reference
      nv -= two_pi * floor(nv * inv_two_pi);
      if (nv <= 0.0) nv += two_pi;
    }
    if (i == 1) nv = fmax(minfreq, fmin(maxfreq, nv));   // the true freq never leaves the clamp range
    if (act) {
      so[t * 7 + i] = nv;                     // (each lane reads and writes only its own column)
      resid = fmax(resid, fabs(d) * inv_scale);
    }
  }
  __syncthreads();
  for (int idx = i; idx < (c1 - c0) * 7; idx += 64) nd[(long long)(c0 + 1) * 7 + idx] = so[idx];
  // one residual row per group (component 0..6, slot 7 = max); k_pll_check reduces them --
  // same-address atomics from thousands of groups would serialise in L2
  double rmax = act ? resid : 0.0;
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, o, 64));
  double *gr = grp_resid + ((long long)s * gridDim.x + grp) * 8;
  if (act) gr[i] = resid;
  if (i == 7) gr[7] = rmax;
}
#endif

// Round bookkeeping, launched right after every integration pass: one 1024-thread block per stream
// reduces (a) the per-workgroup boundary mismatches r of that pass and (b) the per-group Newton
// steps d of the PREVIOUS round's node pass.  The trajectory just written is accepted if it closes
// to rtol by itself, or if the node update that produced its start nodes was already below tol
// (the nodes are then better than tol by the contraction factor).  Accepting here makes all node
// kernels of this round no-ops.
#ifdef FMR_AB_PARTNERS      // seven launches per Newton round (round 1): the partner tests/test_gpu_pll_forms.py compares the product with
__global__ __launch_bounds__(1024) void k_pll_check(IterFlags *fl, int n_streams, double tol,
                                                    const double *__restrict__ grp_resid, int ngrp, int have_d,
                                                    const double *__restrict__ wg_r, int nwg, double rtol) {
  __shared__ double red[16][8];
  __shared__ double redr[16];
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  if (s >= n_streams || fl[s].pll_converged) return;
  const double *gr = grp_resid + (long long)s * ngrp * 8;
  const int comp = tid & 7;
  double r = 0.0;
  if (have_d)
    for (int g = tid >> 3; g < ngrp; g += 128) r = fmax(r, gr[(long long)g * 8 + comp]);
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) r = fmax(r, __shfl_xor(r, o, 64));   // lanes with equal comp
  if ((tid & 63) < 8) red[tid >> 6][comp] = r;
  double rr = 0.0;
  for (int w = tid; w < nwg; w += 1024) rr = fmax(rr, wg_r[(long long)s * nwg + w]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rr = fmax(rr, __shfl_xor(rr, o, 64));
  if ((tid & 63) == 0) redr[tid >> 6] = rr;
  __syncthreads();
  if (tid < 8) {
    double m = 0.0;
#pragma unroll
    for (int w = 0; w < 16; w++) m = fmax(m, red[w][tid]);
    if (tid < 7 && have_d) fl[s].pll_comp[tid] = m;
    if (tid == 7) {
      double mr = 0.0;
#pragma unroll
      for (int w = 0; w < 16; w++) mr = fmax(mr, redr[w]);
      IterFlags &F = fl[s];
      const int it = F.pll_iters;                    // integration passes done before this one
      if (it < 16) F.pll_rhist[it] = mr;
      if (have_d && it >= 1 && it <= 16) F.pll_hist[it - 1] = m;
      F.pll_iters = it + 1;
      if (mr <= rtol) { F.pll_converged = 1; F.pll_r_accepted = 1; F.pll_resid = mr; }
      else if (have_d && m <= tol) { F.pll_converged = 1; F.pll_resid = m; }
      else F.pll_resid = have_d ? m : mr;
    }
  }
}
#endif

// ---------------------------------------------------------------------------
// The same round in three launches instead of seven (integration pass + bookkeeping, up-sweep, down-sweep).
// A launch that depends on the one before it costs ~5 us on this part whatever it does, and a call in lock accepts
// its second pass: 14 of the 23 launches of the seven-kernel form found pll_converged set and left -- ~70 us of a
// 0.8 ms step.  Kernels are merged with the last-arrival pattern: a workgroup publishes its result, fences, takes a
// ticket; whoever draws the last ticket of its set does the next level's work (no workgroup ever waits for another).
//   k_pll_shoot:   integration pass; the last workgroup of a stream does k_pll_check's bookkeeping
//   k_pll_up:      phase A; the last group of every level-2 set composes the set (A2) and stores the running prefix
//                  composites on the way; the last set of a stream walks the level-2 maps (B)
//   k_pll_down:    start delta of a group = its prefix composite applied to the set's start delta (replaces C2's
//                  32-step chain by one 7x8 product), then phase C; residual maxima through 64 x 8 atomicMax slots
// ---------------------------------------------------------------------------
__device__ __forceinline__ void pll_up_from_lds(const PllUpArgs &u, int s, int grp, int n, double *sm, double *sh, int lane) {
  // sm: the group's n Jacobians (49 doubles each), then its mismatches at sm + FMR_NODE_GRP * 49 (stride 7); at least
  // FMR_NODE_GRP2 * 56 doubles long (level 2 stages a set's maps there); sh: 64 doubles
  // Level 1 as a chain (k_pll_up, the chord rounds >= 3 and the A/B partner of the tree in k_pll_shoot's tail)
  double *const sr = sm + FMR_NODE_GRP * 49;
  const int i = lane >> 3, k = lane & 7;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  double val = (act && i == k) ? 1.0 : 0.0;   // P = I, q = 0
  for (int t = 0; t < n; t++) {
    sh[lane] = val;
    __syncthreads();                      // one wave per block: just orders the LDS write
    double acc = (k == 7) ? sr[t * 7 + ii] : 0.0;
    const double *row = sm + t * 49 + ii * 7;
#pragma unroll
    for (int j = 0; j < 7; j++) acc = fma(row[j], sh[j * 8 + k], acc);
    __syncthreads();
    val = acc;
  }
  pll_up_levels23(u, s, grp, val, sm, sh, lane);
}

// Levels 2 and 3 of the up-sweep behind a group's composite (lane i * 8 + k holds P[i][k], k == 7: q[i]); sm: at least
// FMR_NODE_GRP2 * 56 doubles of LDS, sh: 64
__device__ __forceinline__ void pll_up_levels23(const PllUpArgs &u, int s, int grp, double val0, double *sm, double *sh, int lane) {
  const int ngrp = u.ngrp, ngrp2 = u.ngrp2;
  const int i = lane >> 3, k = lane & 7;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  if (act) st_agent(&u.PQ[(((long long)s * ngrp + grp) * 7 + i) * 8 + k], val0);
  // ---- level 2: the last group of the set composes the set
  const int set = grp / FMR_NODE_GRP2;
  const int g0 = set * FMR_NODE_GRP2, g1 = min(g0 + FMR_NODE_GRP2, ngrp);
  if (!pll_last_arrival(u.tick2 + (long long)s * ngrp2 + set, (unsigned int)(g1 - g0))) return;
  {
    const double *pq = u.PQ + (long long)s * ngrp * 56;
    double *pre = u.PRE + (long long)s * ngrp * 56;
    pll_stage_pq<true>(pq, g0, g1 - g0, lane, sm);
    __syncthreads();
    double val = (act && i == k) ? 1.0 : 0.0;
    for (int t = 0; t < g1 - g0; t++) {
      if (act) pre[((long long)(g0 + t) * 7 + i) * 8 + k] = val;     // composite of the groups before g0 + t
      const double *mr = sm + (t * 7 + ii) * 8;
      sh[lane] = val;
      __syncthreads();
      double acc = (k == 7) ? mr[7] : 0.0;
#pragma unroll
      for (int j = 0; j < 7; j++) acc = fma(mr[j], sh[j * 8 + k], acc);
      __syncthreads();
      val = acc;
    }
    if (act) st_agent(&u.PQ2[(((long long)s * ngrp2 + set) * 7 + i) * 8 + k], val);
  }
  // ---- level 3: the last set walks the level-2 maps (lane i = component i)
  if (!pll_last_arrival(&u.sync[s].tick_up, (unsigned int)ngrp2)) return;
  {
    const double *pq2 = u.PQ2 + (long long)s * ngrp2 * 56;
    double *ds = u.dstart2 + (long long)s * ngrp2 * 7;
    const bool a7 = lane < 7;
    const int l7 = a7 ? lane : 0;
    double d = 0.0;
    // the maps of the next batch of 32 are fetched while this one is walked (a memory latency per batch otherwise)
    constexpr int NLQ = (FMR_NODE_GRP2 * 56 + 63) / 64;
    double nxt[NLQ];
    auto fetch = [&](int q0) {
      const int nq = min(FMR_NODE_GRP2, ngrp2 - q0);
      const double *pb = pq2 + (long long)q0 * 56;
#pragma unroll
      for (int v = 0; v < NLQ; v++) { const int idx = lane + 64 * v; nxt[v] = (idx < nq * 56) ? ld_agent(pb + idx) : 0.0; }
    };
    fetch(0);
    for (int q0 = 0; q0 < ngrp2; q0 += FMR_NODE_GRP2) {
      const int nq = min(FMR_NODE_GRP2, ngrp2 - q0);
      __syncthreads();
#pragma unroll
      for (int v = 0; v < NLQ; v++) { const int idx = lane + 64 * v; if (idx < FMR_NODE_GRP2 * 56) sm[idx] = nxt[v]; }
      __syncthreads();
      if (q0 + FMR_NODE_GRP2 < ngrp2) fetch(q0 + FMR_NODE_GRP2);
      for (int t = 0; t < nq; t++) {
        if (a7) ds[(long long)(q0 + t) * 7 + lane] = d;
        const double *row = sm + (t * 7 + l7) * 8;
        const double d0 = readlane_d(d, 0), d1 = readlane_d(d, 1), d2 = readlane_d(d, 2), d3 = readlane_d(d, 3),
                     d4 = readlane_d(d, 4), d5 = readlane_d(d, 5), d6 = readlane_d(d, 6);
        const double p0 = fma(row[0], d0, fma(row[1], d1, row[7]));
        const double p1 = fma(row[2], d2, row[3] * d3);
        const double p2 = fma(row[4], d4, fma(row[5], d5, row[6] * d6));
        d = p0 + (p1 + p2);
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_pll_up(const double *__restrict__ nodes, const double *__restrict__ G,
                                               const double *__restrict__ M, int nck, double *PQ,
                                               double *__restrict__ PRE, double *PQ2, int ngrp2,
                                               double *__restrict__ dstart2, const IterFlags *__restrict__ fl,
                                               PllSync *__restrict__ sync, unsigned int *__restrict__ tick2) {
  // 14.8 KB of LDS in all: ten workgroups per CU, i.e. the ~2500 groups of a 2^27-sample call in ONE round (with the
  // mismatches in an array of their own it was 16.9 KB, nine per CU, and a tenth of the groups ran behind the others)
  __shared__ double sm[FMR_NODE_GRP2 * 56];      // phase A: FMR_NODE_GRP * 49 Jacobian entries, then the mismatches (stride 7)
  __shared__ double sh[64];
  static_assert(FMR_NODE_GRP2 * 56 >= FMR_NODE_GRP * (49 + 7), "shared staging buffer");
  double *const sr = sm + FMR_NODE_GRP * 49;
  const int s = blockIdx.y, grp = blockIdx.x, ngrp = gridDim.x;
  if (fl[s].pll_converged) return;
  const int lane = threadIdx.x;
  const double *nd = nodes + (long long)s * (nck + 1) * 7;
  const double *g = G + (long long)s * nck * 9;
  const double *m = M + (long long)s * nck * 49;
  const int c0 = grp * FMR_NODE_GRP, c1 = min(c0 + FMR_NODE_GRP, nck);
  pll_stage_group(m, g, nd, c0, c1 - c0, lane, sm, sr, nullptr, 7);
  __syncthreads();
  pll_up_from_lds(PllUpArgs{PQ, PRE, PQ2, ngrp, ngrp2, dstart2, sync, tick2}, s, grp, c1 - c0, sm, sh, lane);
}

// The down-sweep of one group of FMR_NODE_GRP chunks (k_pll_down's body, rounds 1-4): start delta of the group = its prefix
// composite applied to the set's start delta, then the deltas propagate chunk by chunk; the new start nodes of chunks
// c0 + 1 .. c0 + n are left in `so` (stride 7) AND stored, the new start node of chunk c0 itself -- which the group before
// this one stores, from its own propagation: the same number up to rounding -- in first[0..6].  Residual maxima through the
// 64 x 8 atomicMax slots.  sm / sr / so: FMR_NODE_GRP x 49 / 7 / 7 doubles of LDS.
__device__ __forceinline__ void pll_down_group(const PllDownArgs &dn, double *nd, const double *g, const double *m, int nck, int s, int grp,
                                               PllSync *sync, double *sm, double *sr, double *so, double *first, int lane) {
  const int i = lane;
  const bool act = i < 7;
  const int ii = act ? i : 0;
  const double two_pi = 2.0 * 3.14159265358979323846, inv_two_pi = 1.0 / two_pi;
  const int c0 = grp * FMR_NODE_GRP, c1 = min(c0 + FMR_NODE_GRP, nck);
  const double *pre = dn.PRE + (((long long)s * dn.ngrp + grp) * 7 + ii) * 8;
  const double *d2 = dn.dstart2 + ((long long)s * dn.ngrp2 + grp / FMR_NODE_GRP2) * 7;
  double pr[8], dv[7];
#pragma unroll
  for (int q = 0; q < 8; q++) pr[q] = pre[q];
#pragma unroll
  for (int q = 0; q < 7; q++) dv[q] = d2[q];
  // scale of the biquad delays: size of the (I,Q) delay pair at the group start
  const double wm = fabs(g[(long long)c0 * 9 + 3]) + fabs(g[(long long)c0 * 9 + 5]);
  double inv_scale = 1.0 / (1e-7 * (wm + 1.0));
  if (i == 0) inv_scale = 1e7; else if (i == 1) inv_scale = 1e9; else if (i == 2) inv_scale = 1e5;
  // the node this group's first chunk was integrated from: NOT read from `nd` -- the group before this one overwrites it in
  // this very launch -- but from the copy the last integration pass left (one per wave: only even groups are asked)
  const double old0 = dn.wave_first[((long long)s * ((nck + 63) / 64) + (grp >> 1)) * 7 + ii];
  pll_stage_group(m, g, nd, c0, c1 - c0, i, sm, sr, so, 7);
  __syncthreads();
  double d = fma(pr[0], dv[0], fma(pr[1], dv[1], pr[7])) + (fma(pr[2], dv[2], pr[3] * dv[3]) +
             fma(pr[4], dv[4], fma(pr[5], dv[5], pr[6] * dv[6])));
  auto fix = [&](double nv) {
    if (i == 0) {                             // keep the phase inside (0, 2 pi] like the reference
      nv -= two_pi * floor(nv * inv_two_pi);
      if (nv <= 0.0) nv += two_pi;
    }
    if (i == 1) nv = fmax(dn.minfreq, fmin(dn.maxfreq, nv));   // the true freq never leaves the clamp range
    return nv;
  };
  if (act) first[i] = (grp == 0) ? old0 : fix(old0 + d);      // (chunk 0 starts from the carried state: fixed)
  double resid = 0.0;
  for (int t = 0; t < c1 - c0; t++) {
    const double *row = sm + t * 49 + ii * 7;
    const double d0 = readlane_d(d, 0), d1 = readlane_d(d, 1), d2v = readlane_d(d, 2), d3 = readlane_d(d, 3),
                 d4 = readlane_d(d, 4), d5 = readlane_d(d, 5), d6 = readlane_d(d, 6);
    const double p0 = fma(row[0], d0, fma(row[1], d1, sr[t * 7 + ii]));
    const double p1 = fma(row[2], d2v, row[3] * d3);
    const double p2 = fma(row[4], d4, fma(row[5], d5, row[6] * d6));
    d = p0 + (p1 + p2);                       // delta of node c+1
    const double nv = fix(so[t * 7 + ii] + d);
    if (act) {
      so[t * 7 + i] = nv;                     // (each lane reads and writes only its own column)
      resid = fmax(resid, fabs(d) * inv_scale);
    }
  }
  __syncthreads();
  for (int idx = i; idx < (c1 - c0) * 7; idx += 64) nd[(long long)(c0 + 1) * 7 + idx] = so[idx];
  // ~40 groups share a slot: same-address atomics from all the groups would serialise in L2
  if (act) atomicMax(&sync[s].dslot[grp & 63][i], pll_max_bits(resid));
}

// The same down-sweep for a wave's two groups at once, as a descent through the tree the Jacobian pass composed them with
// (pll_descend_tree, pll_compose.hpp): five dependent levels instead of two chains of 32 steps, both groups in the same
// rounds (a half-wave each, 28 of its 32 lanes a row of a node).  Lane l owns the node BEHIND its chunk, w0 + l + 1, as the
// chain's groups do: it reads the old one (which no other wave of this launch writes), adds the delta, stores it and keeps it
// as nxt; its own start node is its neighbour's nxt, lane 0's the wave's first (old from wave_first, as in the chain).
// The deltas at the starts of the wave's groups and of the group behind it come from PRE x dstart2; at the call's end there
// is no group behind, and the last chunk's own map gives the end node's delta (one step, one wave of the launch).
// xs: the sample tile.  Staged in two turns: the tree's composites (2 x 15 maps), then the even chunks' maps [M | r] (32).
__device__ __forceinline__ void pll_descend_head(const PllDownArgs &dn, double *nd, const double *g, const double *m, int nck, int s,
                                                 PllSync *sync, double *xs, int lane, double (&sv)[7], double (&nxt)[7]) {
  constexpr int GW = FMR_TREE_SINK * FMR_MAP;            // a group's composites
  constexpr int LFW = FMR_NODE_GRP * FMR_MAP;            // the maps of the wave's 32 even chunks
  constexpr int NU = (2 * GW + 63) / 64, NM = (32 * 49 + 63) / 64, NR = (32 * 7 + 63) / 64;
  static_assert(FMR_NODE_GRP == FMR_TREE_MAXN && 2 * GW <= LFW, "the composites are staged where the even chunks' maps follow");
  double *const de = xs + LFW;                           // [33][7]: deltas at the starts of chunks 0, 2, .. 64 of the wave
  const int w0 = blockIdx.x * 64, nw = min(64, nck - w0), g0 = 2 * blockIdx.x;
  const int half = lane >> 5, l5 = lane & 31;
  const bool valid = lane < nw, at_end = w0 + nw == nck;
  const double two_pi = 2.0 * 3.14159265358979323846, inv_two_pi = 1.0 / two_pi;
  // ---- everything the head reads from memory, in flight together
  const int nup = min(2, dn.ngrp - g0) * GW;
  const double *te = dn.TE + ((long long)s * dn.ngrp + g0) * GW;
  double tu[NU];
#pragma unroll
  for (int u = 0; u < NU; u++) { const int idx = lane + 64 * u; tu[u] = idx < nup ? te[idx] : 0.0; }
  // start deltas of groups g0, g0 + 1 and g0 + 2: lane G * 8 + i, the chain's expression
  const int G = lane >> 3, gi = lane & 7;
  const bool gact = G < 3 && gi < 7 && g0 + G < dn.ngrp;
  double pr[8], dv[7];
  {
    const int grp = gact ? g0 + G : g0;
    const double *pre = dn.PRE + (((long long)s * dn.ngrp + grp) * 7 + (gact ? gi : 0)) * 8;
    const double *d2 = dn.dstart2 + ((long long)s * dn.ngrp2 + grp / FMR_NODE_GRP2) * 7;
#pragma unroll
    for (int q = 0; q < 8; q++) pr[q] = pre[q];
#pragma unroll
    for (int q = 0; q < 7; q++) dv[q] = d2[q];
  }
  double on[7], old0[7], er[8];
  const double *ndn = nd + (long long)(w0 + (valid ? lane : 0) + 1) * 7;
  const double *wf = dn.wave_first + ((long long)s * gridDim.x + blockIdx.x) * 7;
#pragma unroll
  for (int k = 0; k < 7; k++) { on[k] = ndn[k]; old0[k] = wf[k]; }
  const int c0g = min(w0 + 32 * half, nck - 1);          // scale of the biquad delays: the (I,Q) delay pair at the group's start
  const double wm = fabs(g[(long long)c0g * 9 + 3]) + fabs(g[(long long)c0g * 9 + 5]);
  const int ei = lane < 7 ? lane : 0;
  if (at_end) {                                          // the last chunk's map, row per lane
#pragma unroll
    for (int j = 0; j < 7; j++) er[j] = m[(long long)(nck - 1) * 49 + ei * 7 + j];
    er[7] = pll_mismatch(g, nd, nck - 1, ei);
  }
  // ---- upper levels
#pragma unroll
  for (int u = 0; u < NU; u++) { const int idx = lane + 64 * u; if (idx < 2 * GW) xs[idx] = tu[u]; }
  if (gact)
    de[G * 16 * 7 + gi] = fma(pr[0], dv[0], fma(pr[1], dv[1], pr[7])) + (fma(pr[2], dv[2], pr[3] * dv[3]) +
                          fma(pr[4], dv[4], fma(pr[5], dv[5], pr[6] * dv[6])));
  double tm[NM], tr[NR];
  // (the even chunks' maps are asked for once the composites have left the registers: with both held the pass is over 256)
#pragma unroll
  for (int u = 0; u < NM; u++) {
    const int q = lane + 64 * u, p = q / 49, c = w0 + 2 * p;
    tm[u] = (q < 32 * 49 && c < nck) ? m[(long long)c * 49 + (q - 49 * p)] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < NR; u++) {
    const int q = lane + 64 * u, p = q / 7, c = w0 + 2 * p;
    tr[u] = (q < 32 * 7 && c < nck) ? pll_mismatch(g, nd, c, q - 7 * p) : 0.0;
  }
  __syncthreads();
  const int nh = max(0, min(32, nw - 32 * half));
  pll_descend_upper<32>(xs + half * GW, de + half * 16 * 7, nh, l5, [] { __syncthreads(); });
  // ---- leaves: the composites give way to the even chunks' maps (the last barrier above is behind every read of them)
#pragma unroll
  for (int u = 0; u < NM; u++) {
    const int q = lane + 64 * u, p = q / 49, e = q - 49 * p, er_ = e / 7;
    if (q < 32 * 49) xs[p * FMR_MAP + er_ * 8 + (e - 7 * er_)] = tm[u];
  }
#pragma unroll
  for (int u = 0; u < NR; u++) {
    const int q = lane + 64 * u, p = q / 7;
    if (q < 32 * 7) xs[p * FMR_MAP + (q - 7 * p) * 8 + 7] = tr[u];
  }
  __syncthreads();
  pll_descend_leaves<32>(xs + half * 16 * FMR_MAP, de + half * 16 * 7, nh, l5, [] { __syncthreads(); });
  if (at_end) {                                          // the end node's delta: where the delta of chunk nw would stand
    if (lane < 7) {
      double acc = er[7];
#pragma unroll
      for (int j = 0; j < 7; j++) acc = fma(er[j], pll_descend_delta(xs, de, nw - 1, j), acc);
      if (nw & 1) xs[(nw >> 1) * FMR_MAP + lane * 8 + 7] = acc; else de[(nw >> 1) * 7 + lane] = acc;
    }
    __syncthreads();
  }
  // ---- every lane: the node behind its chunk
  auto fix = [&](int k, double nv) {
    if (k == 0) {                             // keep the phase inside (0, 2 pi] like the reference
      nv -= two_pi * floor(nv * inv_two_pi);
      if (nv <= 0.0) nv += two_pi;
    }
    if (k == 1) nv = fmax(dn.minfreq, fmin(dn.maxfreq, nv));   // the true freq never leaves the clamp range
    return nv;
  };
  const double wsc = 1.0 / (1e-7 * (wm + 1.0));
  double resid[7];
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const double d = valid ? pll_descend_delta(xs, de, lane + 1, k) : 0.0;
    nxt[k] = valid ? fix(k, on[k] + d) : 0.0;
    resid[k] = wave_max_d(fabs(d) * (k == 0 ? 1e7 : k == 1 ? 1e9 : k == 2 ? 1e5 : wsc));
    if (valid) nd[(long long)(w0 + lane + 1) * 7 + k] = nxt[k];
    const double first = blockIdx.x == 0 ? old0[k] : fix(k, old0[k] + de[k]);      // (chunk 0 starts from the carried state: fixed)
    const double prev = __shfl_up(nxt[k], 1, 64);
    sv[k] = !valid ? 0.0 : lane == 0 ? first : prev;
  }
  // residual maxima: one slot row per wave (pll_round_check takes the maximum over all of them)
  double rk = 0.0;
#pragma unroll
  for (int k = 0; k < 7; k++) if (lane == k) rk = resid[k];
  if (lane < 7) atomicMax(&sync[s].dslot[blockIdx.x & 63][lane], pll_max_bits(rk));
}

// initial node guess: nominal ramp from the carried state
__global__ void k_pll_begin(double *__restrict__ nodes, ChunkTab ct, const StreamState *st, PllConst pc) {
  const int s = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ct.nck) return;
  const StreamState &S = st[s];
  const double two_pi = 2.0 * 3.14159265358979323846;
  double *nd = nodes + ((long long)s * (ct.nck + 1) + c) * 7;
  long long n0 = 0;
  if (c < ct.nck) n0 = ct.off[c]; else if (ct.nck > 0) n0 = (long long)ct.off[ct.nck - 1] + ct.len[ct.nck - 1];
  // ramp with the mean increment of the previous call: the instantaneous freq carries
  // ~1e-7 rad/sample of loop jitter, which would walk the guess off by ~0.1 rad per 1e6 samples
  const double framp = S.pll_favg_valid ? S.pll_favg : S.pll_freq;
  double ph = S.pll_phase + (double)n0 * framp;
  ph -= two_pi * floor(ph / two_pi);
  if (ph <= 0.0) ph += two_pi;
  if (c == 0) ph = S.pll_phase;
  nd[0] = ph; nd[1] = S.pll_freq; nd[2] = S.lf_x1;
  nd[3] = S.bq_i_x1; nd[4] = S.bq_i_x2; nd[5] = S.bq_q_x1; nd[6] = S.bq_q_x2;
}

// Inclusive prefix sum over the 64 lanes without the LDS crossbar: Hillis-Steele inside each row of 16 (row_shr 1, 2, 4,
// 8, zero fill), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3 (gfx9 DPP).  A ds_bpermute
// shuffle costs > 100 cycles of latency, a DPP step ~10: the per-block walk below is a chain of them.
__device__ __forceinline__ int wave_scan_dpp(int v) {
  auto step = [](int x, auto ctrl, auto rows) {
    return x + __builtin_amdgcn_update_dpp(0, x, decltype(ctrl)::value, decltype(rows)::value, 0xF, true);
  };
  v = step(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xF>{});
  v = step(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xF>{});
  v = step(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xF>{});
  v = step(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xF>{});
  v = step(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});
  v = step(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});
  return v;
}

// After convergence: per-block lock logic (PilotPhaseLock.cpp:154-167), PPS events
// (:133-150) and the state commit.  k_pll_blocks reduces the chunk results to one
// (wrap count, level) pair per block in parallel; k_pll_finish walks the blocks with one
// wave per stream (64 blocks per load, values broadcast through SGPRs).
__global__ void k_pll_blocks(BlockTab bt, ChunkTab ct, const double *__restrict__ G,
                             const int *__restrict__ ck_wraps, int *__restrict__ blk_wraps,
                             double *__restrict__ blk_level, const IterFlags *__restrict__ fl) {
  // a WAVE per block, a lane per chunk (a block of the benchmark holds ~40 chunks): one load per lane and a wave sum, not a
  // thread per block adding its chunks one load behind the other -- this kernel runs beside the next call's front end,
  // where every memory round trip is microseconds
  const int s = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= bt.nb || !fl[s].pll_converged || fl[s].pll_fallback) return;
  const int c0 = ct.first[b], c1 = ct.first[b + 1];
  const double level = (c1 > c0 && lane == 0) ? G[((long long)s * ct.nck + (c1 - 1)) * 9 + 7] : 0.0;
  int w = 0;
  for (int c = c0 + lane; c < c1; c += 64) w += ck_wraps[(long long)s * ct.nck + c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
  if (lane == 0) {
    blk_wraps[(long long)s * bt.nb + b] = w;
    blk_level[(long long)s * bt.nb + b] = level;
  }
}

__global__ __launch_bounds__(64) void k_pll_finish(
    const fm_mpx_t *__restrict__ base, long long base_stride, int base_off, BlockTab bt, ChunkTab ct,
    const float *__restrict__ atan_tab, PllConst pc, int pilot_shift, const double *__restrict__ nodes,
    const double *__restrict__ G, const int *__restrict__ ck_wraps, const unsigned long long *__restrict__ ck_mask,
    int mask_words, const int *__restrict__ blk_wraps, const double *__restrict__ blk_level,
    int *__restrict__ stereo_blk, StreamState *st, const IterFlags *__restrict__ fl,
    const int *__restrict__ walk_go = nullptr) {
  // walk_go != nullptr: the loop state has been committed by k_pll_commit, which also left the call's verdict here -- in
  // the pipelined chain this walk runs behind the NEXT call's tables, whose reset has cleared the round flags by then
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  if (walk_go ? !walk_go[s] : (!fl[s].pll_converged || fl[s].pll_fallback)) return;
  // 6 KB of LDS in all: in the pipelined chain this kernel runs beside the next call's front end, whose workgroup leaves
  // 7.5 KB of a CU's LDS free (with 32 KB it waited for the front end to end, and the next PLL pass behind it)
  constexpr int kFlagBuf = 512;
  __shared__ int sflag[kFlagBuf];
  StreamState &S = st[s];
  int lock_cnt = S.lock_cnt, pilot_periods = S.pilot_periods;
  unsigned long long pps_cnt = S.pps_cnt, sample_cnt = S.sample_cnt;
  int n_pps = 0;
  long long wr = 0, ns = 0;
  // The per-block values come in through LDS, 256 blocks per stage with all of a lane's loads in flight at once: the
  // walk is a chain of cross-lane steps that takes well under a memory latency per batch of 64 blocks, so with the
  // loads inside it -- or one batch ahead of it, as in round 2 -- every batch waited for memory (0.12 / 0.09 ms for
  // 2048 blocks).
  constexpr int kStage = 256;
  __shared__ int s_n[kStage], s_w[kStage];
  __shared__ double s_level[kStage];
  for (int b0 = 0; b0 < bt.nb; b0 += 64) {
    if ((b0 & (kStage - 1)) == 0) {
      __syncthreads();                         // (one wave: orders the LDS accesses of the two stages)
      int vn[kStage / 64], vw[kStage / 64];
      double vl[kStage / 64];
#pragma unroll
      for (int u = 0; u < kStage / 64; u++) {
        const int b = b0 + u * 64 + lane;
        const bool in = b < bt.nb;
        const int bl = in ? b : bt.nb - 1;
        vn[u] = in ? bt.if_len[bl] : 0;
        vw[u] = in ? blk_wraps[(long long)s * bt.nb + bl] : 0;
        vl[u] = blk_level[(long long)s * bt.nb + bl];
      }
#pragma unroll
      for (int u = 0; u < kStage / 64; u++) { s_n[u * 64 + lane] = vn[u]; s_w[u * 64 + lane] = vw[u]; s_level[u * 64 + lane] = vl[u]; }
      __syncthreads();
    }
    const int cnt = min(64, bt.nb - b0);
    const bool mine = lane < cnt;
    const int my_n = s_n[(b0 & (kStage - 1)) + lane], my_w = s_w[(b0 & (kStage - 1)) + lane];
    const double my_level = s_level[(b0 & (kStage - 1)) + lane];
    const bool my_ok = (2 * my_level > pc.minsignal) || my_n == 0;    // block keeps the lock (or is empty)
    int my_flag = 0;
    // one block through the reference's per-block logic (PilotPhaseLock.cpp:133-167)
    auto one_block = [&](int j) {
      const int b = b0 + j;
      const int n = __builtin_amdgcn_readlane(my_n, j);
      const int w = __builtin_amdgcn_readlane(my_w, j);
      const double level = readlane_d(my_level, j);
      if (n == 0) { if (lane == j) my_flag = (lock_cnt >= pc.lock_delay); return; }
      const bool was_locked = (lock_cnt >= pc.lock_delay);
      const int pps_blk_start = n_pps;
      if (pilot_periods + w >= pc.pilot_frequency) {
        // the 19000th period ends inside this block: find the chunk and the sample from the wrap masks
        int kth = pc.pilot_frequency - pilot_periods;      // the kth wrap of this block (1-based)
        const int after = w - kth;                          // wraps of the block after the event
        // the chunk that holds it: 64 chunks per step (prefix sum of their wrap counts across the wave) instead of a
        // chain of dependent loads, one per chunk -- ~20 of them per event, 13 events per 2048-block call
        const int cf0 = ct.first[b], cf1 = ct.first[b + 1];
        for (int cb = cf0; cb < cf1; cb += 64) {
          const int cw_l = (cb + lane < cf1) ? ck_wraps[(long long)s * ct.nck + cb + lane] : 0;
          const int pre = wave_scan_dpp(cw_l);              // inclusive
          const int tot = __builtin_amdgcn_readlane(pre, 63);
          if (kth > tot) { kth -= tot; continue; }
          const int hit = __ffsll((long long)__ballot(pre >= kth)) - 1;
          kth -= __builtin_amdgcn_readlane(pre, hit) - __builtin_amdgcn_readlane(cw_l, hit);
          const int c = cb + hit;
          const unsigned long long *mk = ck_mask + ((long long)s * ct.nck + c) * mask_words;
          int q = -1;
          for (int wd = 0; wd < mask_words && q < 0; wd++) {
            unsigned long long m = mk[wd];
            const int pc_ = __popcll(m);
            if (kth > pc_) { kth -= pc_; continue; }
            for (int t = 1; t < kth; t++) m &= m - 1;       // drop the kth-1 lowest set bits
            q = wd * 64 + (__ffsll((long long)m) - 1);
          }
          if (was_locked) {
            const int ib = ct.off[c] - bt.if_off[b] + q;   // index inside the block
            if (n_pps < FMR_MAX_PPS && lane == 0) {
              PpsEventDev &ev = S.pps[n_pps];
              ev.pps_index = pps_cnt;
              ev.sample_index = sample_cnt + (unsigned long long)ib;
              ev.block_position = (double)ib / (double)n;
              ev.block = (unsigned)b;
            }
            n_pps++;
            pps_cnt++;
          }
          break;
        }
        pilot_periods = after;
      } else {
        pilot_periods += w;
      }
      wr += w; ns += n;
      if (2 * level > pc.minsignal) {
        if (lock_cnt < pc.lock_delay) lock_cnt += n;
      } else {
        lock_cnt = 0;
      }
      if (lock_cnt < pc.lock_delay) {
        pilot_periods = 0;
        pps_cnt = 0;
        n_pps = pps_blk_start;
      }
      sample_cnt += (unsigned long long)n;
      if (lane == j) my_flag = (lock_cnt >= pc.lock_delay);
    };
    int pos = 0;
    while (pos < cnt) {
      if (lock_cnt < pc.lock_delay) { one_block(pos); pos++; continue; }   // acquiring: block by block
      // locked: every following block that keeps the lock and does not complete the 19000th
      // period only advances the counters -> take the whole run at once
      const bool in_run = mine && lane >= pos;
      const int pw = wave_scan_dpp(in_run ? my_w : 0);     // inclusive prefix sum of the wraps from pos
      const bool stop = in_run && (!my_ok || pilot_periods + pw >= pc.pilot_frequency);
      const unsigned long long sm = __ballot(stop);
      const int run_end = sm ? (__ffsll((long long)sm) - 1) : cnt;   // first block that needs the full logic
      if (run_end > pos) {
        const bool take = in_run && lane < run_end;
        // totals of the run: last lane of a DPP scan (a block holds <= 2^24 samples, 64 of them fit an int)
        const int sw = __builtin_amdgcn_readlane(wave_scan_dpp(take ? my_w : 0), 63);
        const long long sn = __builtin_amdgcn_readlane(wave_scan_dpp(take ? my_n : 0), 63);
        pilot_periods += sw; wr += sw; ns += sn; sample_cnt += (unsigned long long)sn;
        if (take) my_flag = 1;
      }
      pos = run_end;
      if (pos < cnt) { one_block(pos); pos++; }
    }
    // the flags leave through LDS: a global store inside the loop would put its round trip into the wait for the
    // next batch's prefetched values (vmcnt counts loads and stores alike)
    sflag[(b0 & (kFlagBuf - 1)) + lane] = my_flag;
    if (((b0 + 64) & (kFlagBuf - 1)) == 0 || b0 + 64 >= bt.nb) {
      const int f0 = b0 & ~(kFlagBuf - 1);
      for (int q = lane; q < min(kFlagBuf, bt.nb - f0); q += 64) stereo_blk[(long long)s * bt.nb + f0 + q] = sflag[q];
    }
  }
  if (lane != 0) return;
  if (ct.nck > 0 && !walk_go) {
    const double *g = G + ((long long)s * ct.nck + (ct.nck - 1)) * 9;
    if (ns >= 65536) {
      S.pll_favg = ((double)wr * 2.0 * 3.14159265358979323846 + (g[0] - S.pll_phase)) / (double)ns;
      S.pll_favg_valid = (lock_cnt >= pc.lock_delay) ? 1 : 0;
    }
    S.pll_phase = g[0]; S.pll_freq = g[1]; S.lf_x1 = g[2];
    S.bq_i_x1 = g[3]; S.bq_i_x2 = g[4]; S.bq_q_x1 = g[5]; S.bq_q_x2 = g[6];
    S.pll_level = g[7]; S.pll_freq_err = g[8];
  }
  S.lock_cnt = lock_cnt; S.pilot_periods = pilot_periods; S.pps_cnt = pps_cnt; S.sample_cnt = sample_cnt;
  S.n_pps = n_pps < FMR_MAX_PPS ? n_pps : FMR_MAX_PPS;
  S.stereo_detected = (lock_cnt >= pc.lock_delay);
}

// Pipelined chain: the part of k_pll_finish the NEXT call's PLL needs -- the loop state at the end of the call and the
// mean phase increment its start nodes are ramped with -- without the walk over the blocks.  The walk's two inputs to it
// are sums (wraps, samples) and whether the call ends in lock: the lock counter restarts at every block below the
// signal threshold and counts samples until it reaches the delay, so it ends at or above the delay exactly when the
// samples behind the last such block (with the carried count when there is none) reach it.  One wave per stream, two
// passes over the block values with every load of a pass in flight.  The walk then runs a call late, behind the next
// call's tables: on the side stream it was between this call's PLL and those tables -- 0.06 ms alone, 0.19 ms when it
// shares a compute unit with the next front end, which is that front end's whole duration -- and the next call's first
// PLL pass waited for it.
// Beside the next call's front end a memory round trip takes microseconds (the front end keeps HBM at 60% of its peak):
// a lane per block with its loads one behind the other was 64 round trips, 0.19 ms.  Here a thread holds eight blocks and
// has all their loads in flight at once: three round trips for up to 2048 blocks.
#define FMR_COMMIT_THREADS 256
__global__ __launch_bounds__(FMR_COMMIT_THREADS) void k_pll_commit(BlockTab bt, ChunkTab ct, PllConst pc,
                                                                   const double *__restrict__ G,
                                                                   const int *__restrict__ blk_wraps,
                                                                   const double *__restrict__ blk_level, StreamState *st,
                                                                   const IterFlags *__restrict__ fl,
                                                                   int *__restrict__ walk_go) {
  constexpr int NT = FMR_COMMIT_THREADS, K = 8;
  __shared__ int s_low[NT / 64];
  __shared__ long long s_sum[NT / 64][3];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool go = fl[s].pll_converged && !fl[s].pll_fallback;
  if (tid == 0) walk_go[s] = go ? 1 : 0;
  if (!go || ct.nck <= 0) return;
  StreamState &S = st[s];
  const int lock0 = S.lock_cnt;
  const double ph0 = S.pll_phase;
  double gl[9];
  if (tid == 0) {
    const double *g = G + ((long long)s * ct.nck + (ct.nck - 1)) * 9;
#pragma unroll
    for (int q = 0; q < 9; q++) gl[q] = g[q];
  }
  // pass 1: the last block below the signal threshold
  int last_low = -1;
  for (int b0 = 0; b0 < bt.nb; b0 += NT * K) {
    int n[K]; double lv[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int b = min(b0 + j * NT + tid, bt.nb - 1);
      n[j] = bt.if_len[b]; lv[j] = blk_level[(long long)s * bt.nb + b];
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int b = b0 + j * NT + tid;
      if (b < bt.nb && n[j] != 0 && !(2 * lv[j] > pc.minsignal)) last_low = max(last_low, b);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) last_low = max(last_low, __shfl_xor(last_low, o, 64));
  if (lane == 0) s_low[wv] = last_low;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < NT / 64; u++) last_low = max(last_low, s_low[u]);
  // pass 2: wraps, samples, samples behind that block
  long long wr = 0, ns = 0, ns_after = 0;
  for (int b0 = 0; b0 < bt.nb; b0 += NT * K) {
    int n[K], w[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int b = min(b0 + j * NT + tid, bt.nb - 1);
      n[j] = bt.if_len[b]; w[j] = blk_wraps[(long long)s * bt.nb + b];
    }
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int b = b0 + j * NT + tid;
      if (b < bt.nb && n[j] != 0) { wr += w[j]; ns += n[j]; if (b > last_low) ns_after += n[j]; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wr += __shfl_xor(wr, o, 64); ns += __shfl_xor(ns, o, 64); ns_after += __shfl_xor(ns_after, o, 64);
  }
  if (lane == 0) { s_sum[wv][0] = wr; s_sum[wv][1] = ns; s_sum[wv][2] = ns_after; }
  __syncthreads();
  if (tid != 0) return;
  wr = ns = ns_after = 0;
#pragma unroll
  for (int u = 0; u < NT / 64; u++) { wr += s_sum[u][0]; ns += s_sum[u][1]; ns_after += s_sum[u][2]; }
  const long long cnt_end = (last_low < 0 ? (long long)lock0 : 0ll) + ns_after;
  if (ns >= 65536) {
    S.pll_favg = ((double)wr * 2.0 * 3.14159265358979323846 + (gl[0] - ph0)) / (double)ns;
    S.pll_favg_valid = (cnt_end >= (long long)pc.lock_delay) ? 1 : 0;
  }
  S.pll_phase = gl[0]; S.pll_freq = gl[1]; S.lf_x1 = gl[2];
  S.bq_i_x1 = gl[3]; S.bq_i_x2 = gl[4]; S.bq_q_x1 = gl[5]; S.bq_q_x2 = gl[6];
  S.pll_level = gl[7]; S.pll_freq_err = gl[8];
}

// Serial fallback: the plain loop when the shooting iteration did not converge (unlocked: without a pilot the loop's
// state is not a function of the recent input and nothing along time can be decomposed, NOTEBOOK.md).
// Round 4: one WAVE per stream.  A lone wave issues an instruction every ~4.8 cycles whatever it is, and the round-3
// loop was 150 instructions per sample (720 cycles): a third of them the sin / cos of the phase.  Here the pair
// (sin, cos) is carried along: turned by the phase increment of the sample (whose sine and cosine are fourth-order
// polynomials around the middle of the 60 Hz wide frequency range, eight fused multiply-adds) and set again from
// pll_sincos at the head of every run of 64 samples, so that it is never more than 64 rotations (1e-14) from it.
// The 64 samples of a run arrive with one load and leave with one store (v_readlane in, a select per sample out),
// wraps and PPS bookkeeping are scalar branches.  Everything else is the reference's arithmetic as in pll_step<false>.
template <bool PILOT_SHIFT>
__global__ __launch_bounds__(64) void k_pll_fallback(
    const fm_mpx_t *__restrict__ base, long long base_stride, int base_off, BlockTab bt,
    double *__restrict__ raw, long long raw_stride, int raw_off, const float *__restrict__ atan_tab,
    PllConst pc, int *__restrict__ stereo_blk, StreamState *st, int n_streams, IterFlags *fl) {
  __shared__ float tab[257];
  for (int i = threadIdx.x; i < 257; i += blockDim.x) tab[i] = atan_tab[i];
  __syncthreads();
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= n_streams || fl[s].pll_converged) return;
  if (lane == 0) fl[s].pll_fallback = 1;
  StreamState &S = st[s];
  // (every lane holds the same state and runs the same chain: the values are wave-uniform)
  double phase = S.pll_phase, freq = S.pll_freq, lf1 = S.lf_x1;
  double wi1 = S.bq_i_x1, wi2 = S.bq_i_x2, wq1 = S.bq_q_x1, wq2 = S.bq_q_x2;
  double li = S.pll_level, lq = 0.0, freq_err = S.pll_freq_err;
  int lock_cnt = S.lock_cnt, pilot_periods = S.pilot_periods;
  unsigned long long pps_cnt = S.pps_cnt, sample_cnt = S.sample_cnt;
  int n_pps = 0;
  long long wr = 0, ns = 0;
  double ph_start = S.pll_phase;
  bool favg_locked = (S.lock_cnt >= pc.lock_delay);
  const fm_mpx_t *xin = base + (long long)s * base_stride + base_off;
  double *out = raw + (long long)s * raw_stride + raw_off;
  const double two_pi = 2.0 * 3.14159265358979323846;
  const PllRot rot = pll_rot_make(pc);
  const double fminv = pc.minfreq, fmaxv = pc.maxfreq;
  for (int b = 0; b < bt.nb; b++) {
    const int n = bt.if_len[b];
    if (n == 0) { if (lane == 0) stereo_blk[(long long)s * bt.nb + b] = (lock_cnt >= pc.lock_delay); continue; }
    const int off = bt.if_off[b];
    const bool was_locked = (lock_cnt >= pc.lock_delay);
    // the mean phase increment that seeds the next call's node guess is measured over locked signal only, and over
    // the last quarter of a long call: the pull-in transient would put it off by far more than the ~1e-9
    // rad/sample the ramp guess tolerates over millions of samples
    if ((was_locked && !favg_locked) || b == (bt.nb * 3) / 4) { wr = 0; ns = 0; ph_start = phase; }
    favg_locked = was_locked;
    const int pps_blk_start = n_pps;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int cnt = min(64, n - i0);
      const double xv = (lane < cnt) ? (double)xin[off + i0 + lane] : 0.0;
      double psin, pcos;
      pll_sincos(phase, psin, pcos);           // exact at the head of every run of 64 samples
      double ov = 0.0;
      // one sample; (w1, w2) are the biquad delays (newest, older) on entry -- the new value is written over the OLDER
      // one, so the caller swaps the roles instead of the kernel moving registers
      auto step = [&](int u, double &wi_1, double &wi_2, double &wq_1, double &wq_2) {
        const double x = readlane_d(xv, u);
        // PilotPhaseLock.cpp:73-151, the arithmetic of pll_step<false>
        const double carrier = PILOT_SHIFT ? (2 * pcos * pcos - 1) : (2 * psin * pcos);
        const double o = (carrier * x) * 2.0;
        ov = (lane == u) ? o : ov;
        const double phasor_i = psin * x, phasor_q = pcos * x;
        const double wi0 = phasor_i - (pc.bq_a1 * wi_1 + pc.bq_a2 * wi_2);
        const double wq0 = phasor_q - (pc.bq_a1 * wq_1 + pc.bq_a2 * wq_2);
        const double new_i = pc.bq_b0 * wi0, new_q = pc.bq_b0 * wq0;
        const double e = (double)fast_atan2f_dev((float)new_q, (float)new_i, tab);
        li = new_i; lq = new_q;
        const double y = pc.lf_b0 * e + pc.lf_b1 * lf1;
        freq_err = y;
        const double f_un = freq + y;
        // fmax(minfreq, fmin(maxfreq, f_un)) without the two canonicalising v_max the compiler puts in front of a
        // constant operand it cannot prove quiet (same instructions, same result: v_min / v_max return the other operand
        // for a NaN)
        double f_new;
        asm("v_min_f64 %0, %1, %2" : "=v"(f_new) : "v"(f_un), "s"(fmaxv));
        asm("v_max_f64 %0, %1, %2" : "=v"(f_new) : "v"(f_new), "s"(fminv));
        lf1 = e;
        wi_2 = wi0; wq_2 = wq0;
        freq = f_new;
        phase = phase + f_new;
        pll_rotate(psin, pcos, f_new, rot);       // sin / cos of the next phase
        if (__ballot(phase > two_pi) != 0ull) {       // (wave-uniform: a scalar branch)
          phase -= two_pi;
          pilot_periods++;
          wr++;
          if (pilot_periods == pc.pilot_frequency) {
            pilot_periods = 0;
            if (was_locked) {
              if (n_pps < FMR_MAX_PPS && lane == 0) {
                PpsEventDev &ev = S.pps[n_pps];
                ev.pps_index = pps_cnt;
                ev.sample_index = sample_cnt + (unsigned long long)(i0 + u);
                ev.block_position = (double)(i0 + u) / (double)n;
                ev.block = (unsigned)b;
              }
              n_pps++;
              pps_cnt++;
            }
          }
        }
      };
      int u = 0;
      for (; u + 2 <= cnt; u += 2) { step(u, wi1, wi2, wq1, wq2); step(u + 1, wi2, wi1, wq2, wq1); }
      if (u < cnt) {
        step(u, wi1, wi2, wq1, wq2);
        const double ti = wi1, tq = wq1;
        wi1 = wi2; wi2 = ti; wq1 = wq2; wq2 = tq;
      }
      if (lane < cnt) out[off + i0 + lane] = ov;
    }
    if (2 * sqrt((li * li) + (lq * lq)) > pc.minsignal) {
      if (lock_cnt < pc.lock_delay) lock_cnt += n;
    } else {
      lock_cnt = 0;
    }
    if (lock_cnt < pc.lock_delay) { pilot_periods = 0; pps_cnt = 0; n_pps = pps_blk_start; }
    sample_cnt += (unsigned long long)n;
    ns += n;
    if (lane == 0) stereo_blk[(long long)s * bt.nb + b] = (lock_cnt >= pc.lock_delay);
  }
  if (lane != 0) return;
  if (ns >= 65536) {
    S.pll_favg = ((double)wr * 2.0 * 3.14159265358979323846 + (phase - ph_start)) / (double)ns;
    S.pll_favg_valid = (lock_cnt >= pc.lock_delay) ? 1 : 0;
  }
  S.pll_phase = phase; S.pll_freq = freq; S.lf_x1 = lf1;
  S.bq_i_x1 = wi1; S.bq_i_x2 = wi2; S.bq_q_x1 = wq1; S.bq_q_x2 = wq2;
  S.pll_level = sqrt((li * li) + (lq * lq)); S.pll_freq_err = freq_err;
  S.lock_cnt = lock_cnt; S.pilot_periods = pilot_periods; S.pps_cnt = pps_cnt; S.sample_cnt = sample_cnt;
  S.n_pps = n_pps < FMR_MAX_PPS ? n_pps : FMR_MAX_PPS;
  S.stereo_detected = (lock_cnt >= pc.lock_delay);
}

}  // namespace fmr
