// kernels_iqcorr.hpp -- DC-offset and IQ-imbalance correction on the capture, ahead of the blanker and of every front end
// (fmr_enable_iq_correction).  The definitions are in include/fmradion_amd.h;
// tests/iqcorr_fixture.py restates them in numpy.
//
// Indices, intervals and pieces are the blanker's (kernels_blanker.hpp): sample n counts from the chain's first sample,
// interval j = [j Q, (j + 1) Q), Q = kNbQ = 4096, a call hands in [n0, n1) of every row and a piece is the part of one
// interval inside the call.  The streaming kernels have one workgroup per (piece, row) and walk the piece in 16-byte
// pairs exactly as the blanker's do (NbWalk, nb_load_pair).
//
//   k_iqc_moments  classifies each sample of the piece (non-finite, skipped: finite with p > 4, usable) and sums the five
//                  integer moments of the usable ones: int64 per lane, a wave reduction by shuffles, the four waves through
//                  LDS.  One IqcPart per piece.  Integer sums: any order gives the same bits.
//   k_iqc_coef     one workgroup per (tile of 512 pieces, row), one piece per thread.  It continues the row's running
//                  totals Tot[j] = sum of the intervals before j: Tot[j0] comes from the ring, the pieces more than two
//                  tiles in front are summed again by every workgroup (a strided block reduction: no workgroup waits
//                  for another), three block scans cover the two tiles before and the own tile.  The window of interval j is
//                  Tot[j] - Tot[j - c]; the coefficients follow in fp64, one rounding per operation, and go into the
//                  piece's part with a refused flag.  The totals behind the call's complete intervals go into the ring:
//                  the slots a launch writes (j0 + 1 .. j0 + pieces) are none of those it reads (j0 - W .. j0), the ring
//                  has at least pieces + W + 2 slots.  The open interval is kept twice, by call parity: read parity ^ 1,
//                  write parity.
//   k_iqc_apply    FMR_IQC_ACT only: y = z - w conj(z), z = x - d, in fp32 with every product and sum rounded, with the
//                  piece's coefficients (uniform per workgroup); a non-finite sample, and every sample of a piece whose
//                  coefficients are all zero, passes bit for bit.  16-byte loads and stores; no LDS, no atomics.
//   k_iqc_records  one wave per row, off the front end's path: the parts of the call in interval order into the row's open
//                  record (kept in place: only this wave touches it), a complete record to ring slot (index mod L).
//
// Nothing here waits on another workgroup or on the host; every value is written with plain vector stores.  The
// translation unit is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_blanker.hpp"

namespace fmr {

constexpr int kIqcMaxW = 1024;
constexpr int kIqcCoefT = 512;       // threads of k_iqc_coef = pieces of a tile
constexpr int kIqcBack = kIqcMaxW / kIqcCoefT;     // tiles a window reaches back at most
static_assert(kIqcBack * kIqcCoefT == kIqcMaxW, "whole tiles");

// fmr_iq_correction_record, field for field (the stage checks the size)
struct IqcRec {
  uint64_t index, first_interval;
  uint64_t n_usable, n_nonfinite, n_skipped, n_refused;
  int64_t sum_re, sum_im, sum_rr, sum_ii, sum_ri;
  uint32_t n_intervals;
  float dc_re, dc_im, w_re, w_im;
  uint32_t reserved;
};

// the six exact sums: of one piece, of an interval, or running (wrap-around is harmless: only differences are used)
struct IqcSum {
  long long n, s[5];          // usable samples; S_r, S_i, S_rr, S_ii, S_ri
  __device__ __forceinline__ void add(const IqcSum &o) {
    n += o.n;
#pragma unroll
    for (int q = 0; q < 5; q++) s[q] += o.s[q];
  }
  __device__ __forceinline__ void sub(const IqcSum &o) {
    n -= o.n;
#pragma unroll
    for (int q = 0; q < 5; q++) s[q] -= o.s[q];
  }
};

// one piece: k_iqc_moments leaves the sums and the counts, k_iqc_coef the coefficients and the flag
struct IqcPart {
  IqcSum m;
  unsigned nnon, nskip;
  float dr, di, wr, wi;       // applied coefficients of the piece's interval
  unsigned refused, pad;
};

struct IqcCoef {
  int W, R, L, act;
  int dc, balance;            // which part is applied
};

// what a row carries from call to call besides the ring of running totals
struct IqcState {
  IqcSum open[2];             // by call parity: the sums of the open interval in front of the next call
  IqcRec rec;                 // the open record (k_iqc_records alone)
};

__device__ __forceinline__ bool iqc_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }       // false for NaN and Inf
__device__ __forceinline__ long long iqc_fix(float v) { return (long long)floor((double)v * 68719476736.0); }   // floor(v 2^36)

// one sample into the lane's sums
__device__ __forceinline__ void iqc_take(float re, float im, IqcSum &m, unsigned &nnon, unsigned &nskip) {
  if (!iqc_finite(re) || !iqc_finite(im)) { nnon++; return; }
  if (!(nb_power(re, im) <= 4.f)) { nskip++; return; }
  m.n++;
  m.s[0] += iqc_fix(re);
  m.s[1] += iqc_fix(im);
  m.s[2] += iqc_fix(__fmul_rn(re, re));
  m.s[3] += iqc_fix(__fmul_rn(im, im));
  m.s[4] += iqc_fix(__fmul_rn(re, im));
}

// ---- moments ----
// iq + row stride: sample n0 of the row.  part[row pmax + piece].
__global__ __launch_bounds__(kNbT) void k_iqc_moments(const float2 *__restrict__ iq, long long stride, long long n0, long long n1,
                                                      int pmax, IqcPart *__restrict__ part) {
  __shared__ long long r_s[kNbT / 64][6];
  __shared__ unsigned r_c[kNbT / 64][2];
  const int tid = threadIdx.x, row = blockIdx.y;
  const long long j = n0 / kNbQ + blockIdx.x;
  const long long lo = j * kNbQ > n0 ? j * kNbQ : n0, hi = (j + 1) * kNbQ < n1 ? (j + 1) * kNbQ : n1;
  const long long a = lo - n0, b = hi - n0;
  const float2 *x = iq + (long long)row * stride;
  const NbWalk w(x, a);
  nb_v4f v[kNbPairs];
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) v[k] = nb_load_pair(x, w.i0(tid, k), a, b);
  IqcSum m{};
  unsigned nnon = 0, nskip = 0;
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) {
    const long long i0 = w.i0(tid, k);
    if (i0 >= a && i0 < b) iqc_take(v[k].x, v[k].y, m, nnon, nskip);
    if (i0 + 1 >= a && i0 + 1 < b) iqc_take(v[k].z, v[k].w, m, nnon, nskip);
  }
  for (int d = 32; d > 0; d >>= 1) {
    m.n += __shfl_xor(m.n, d);
#pragma unroll
    for (int q = 0; q < 5; q++) m.s[q] += __shfl_xor(m.s[q], d);
    nnon += __shfl_xor(nnon, d); nskip += __shfl_xor(nskip, d);
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    r_s[wave][0] = m.n;
#pragma unroll
    for (int q = 0; q < 5; q++) r_s[wave][1 + q] = m.s[q];
    r_c[wave][0] = nnon; r_c[wave][1] = nskip;
  }
  __syncthreads();
  if (tid == 0) {
    IqcPart o{};
    for (int u = 0; u < kNbT / 64; u++) {
      o.m.n += r_s[u][0];
#pragma unroll
      for (int q = 0; q < 5; q++) o.m.s[q] += r_s[u][1 + q];
      o.nnon += r_c[u][0]; o.nskip += r_c[u][1];
    }
    part[(size_t)row * pmax + blockIdx.x] = o;
  }
}

// The coefficients of an interval from its window sums (c = 0: an empty window), fp64, one rounding per operation, in the
// header's order.  Returns the refused flag.
__device__ inline unsigned iqc_solve(const IqcSum &win, const IqcCoef &cf, float &dr, float &di, float &wr, float &wi) {
  dr = di = wr = wi = 0.f;
  if (win.n < kNbQ / 2) return 0u;
  const double r = __ddiv_rn(1.0, __dmul_rn((double)win.n, 68719476736.0));
  const double m_r = __dmul_rn((double)win.s[0], r), m_i = __dmul_rn((double)win.s[1], r);
  const double E_rr = __dmul_rn((double)win.s[2], r), E_ii = __dmul_rn((double)win.s[3], r), E_ri = __dmul_rn((double)win.s[4], r);
  const double P = __dsub_rn(__dadd_rn(E_rr, E_ii), __dadd_rn(__dmul_rn(m_r, m_r), __dmul_rn(m_i, m_i)));
  const double C_r = __dsub_rn(__dsub_rn(E_rr, E_ii), __dsub_rn(__dmul_rn(m_r, m_r), __dmul_rn(m_i, m_i)));
  const double C_i = __dsub_rn(__dmul_rn(2.0, E_ri), __dmul_rn(2.0, __dmul_rn(m_r, m_i)));
  const double D = __dsub_rn(__dmul_rn(P, P), __dadd_rn(__dmul_rn(C_r, C_r), __dmul_rn(C_i, C_i)));
  double w_r = 0.0, w_i = 0.0;
  unsigned refused = 0;
  if (P > 9.094947017729282e-13 && D > 0.0) {        // 2^-40
    const double t = __dadd_rn(P, __dsqrt_rn(D));
    w_r = __ddiv_rn(C_r, t); w_i = __ddiv_rn(C_i, t);
    if (__dadd_rn(__dmul_rn(w_r, w_r), __dmul_rn(w_i, w_i)) > 0.0625) { w_r = 0.0; w_i = 0.0; refused = 1; }
  }
  if (cf.dc) { dr = (float)m_r; di = (float)m_i; }
  if (cf.balance) { wr = (float)w_r; wi = (float)w_i; }
  return refused;
}

// ---- coefficients ----
// inclusive scan of one IqcSum per thread over the workgroup: by shuffles inside the wave, the waves' totals through
// s_wave (kIqcCoefT / 64 entries); total = the sum over the workgroup
__device__ inline IqcSum iqc_block_scan(IqcSum v, IqcSum *s_wave, IqcSum &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    IqcSum t;
    t.n = __shfl_up(v.n, d);
#pragma unroll
    for (int q = 0; q < 5; q++) t.s[q] = __shfl_up(v.s[q], d);
    if (lane >= d) v.add(t);
  }
  __syncthreads();                         // (s_wave may still be read from the scan before)
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  total = IqcSum{};
  for (int u = 0; u < kIqcCoefT / 64; u++) {
    if (u == wave) v.add(total);
    total.add(s_wave[u]);
  }
  return v;
}

// One workgroup per (tile of T = kIqcCoefT pieces, row); thread tid owns piece k0 + tid, k0 = tile T.  With
// Tot[j0 + k] = Tot[j0] + the sums of the pieces before k (the first on top of the carried open interval):
//   base   Tot[j0 + max(k0 - B T, 0)], B = kIqcBack: Tot[j0] from the ring and a strided block reduction over the pieces
//          in front (a window reaches back W <= B T intervals)
//   scans  one per chunk of T pieces: the B chunks before the tile, then the tile
//   tot    this workgroup's own scratch of (B + 1) T + 1 totals, tot[e] = Tot[j0 + k0 - B T + e]: written, one barrier, read
// part[row pmax + piece] (this call's parity); tot_all[(row tiles + tile) ((B + 1) T + 1) + e]; ring[row (rmask + 1) + (j & rmask)].
__global__ __launch_bounds__(kIqcCoefT) void k_iqc_coef(IqcPart *__restrict__ part_all, int pmax, long long n0, long long n1,
                                                        int par, IqcSum *tot_all, IqcSum *ring_all, int rmask,
                                                        IqcState *__restrict__ state, IqcCoef cf) {
  constexpr int T = kIqcCoefT, B = kIqcBack;
  __shared__ IqcSum s_wave[T / 64];
  const int tid = threadIdx.x, tile = blockIdx.x, row = blockIdx.y;
  const long long j0 = n0 / kNbQ;
  const int P = (int)((n1 - 1) / kNbQ - j0 + 1);
  IqcPart *part = part_all + (size_t)row * pmax;
  IqcSum *tot = tot_all + ((size_t)row * gridDim.x + tile) * ((B + 1) * T + 1);
  IqcSum *ring = ring_all + (size_t)row * (rmask + 1);
  const IqcSum open_prev = state[row].open[par ^ 1];
  const int k0 = tile * T, kb = k0 >= B * T ? k0 - B * T : 0;        // the scans start at piece kb
  auto full = [&](int k) {                 // the sums of piece k, the call's first on top of the open interval
    IqcSum v = part[k].m;
    if (k == 0) v.add(open_prev);
    return v;
  };
  IqcSum run{};
  for (int q = tid; q < kb; q += T) run.add(full(q));
  iqc_block_scan(run, s_wave, run);
  run.add(ring[j0 & rmask]);               // Tot[j0 + kb]
  IqcSum mine{}, own{};                    // Tot[j0 + k] and the sums of the own piece
#pragma unroll 1
  for (int ch = 0; ch <= B; ch++) {
    const int kk = k0 - (B - ch) * T + tid;
    const IqcSum v = kk >= 0 && kk < P ? full(kk) : IqcSum{};
    IqcSum total;
    IqcSum inc = iqc_block_scan(v, s_wave, total);
    inc.add(run);
    if (ch == B && tid == T - 1) tot[(B + 1) * T] = inc;
    inc.sub(v);
    tot[ch * T + tid] = inc;
    if (ch == B) { mine = inc; own = v; }
    run.add(total);
  }
  __syncthreads();
  const int k = k0 + tid;
  if (k >= P) return;
  const long long j = j0 + k;
  const int c = j < cf.W ? (int)j : cf.W;
  IqcSum win{};
  if (c > 0) {
    win = mine;
    const long long f = j - c;
    win.sub(f >= j0 ? tot[B * T + tid - c] : ring[f & rmask]);
  }
  float dr, di, wr, wi;
  const unsigned refused = iqc_solve(win, cf, dr, di, wr, wi);
  part[k].dr = dr; part[k].di = di; part[k].wr = wr; part[k].wi = wi; part[k].refused = refused;
  const bool complete = (j + 1) * kNbQ <= n1;
  if (complete) ring[(j + 1) & rmask] = tot[B * T + tid + 1];
  if (k == P - 1) state[row].open[par] = complete ? IqcSum{} : own;
}

// ---- apply ----
// iq / stride as above; out / ostride the corrected rows (same 16-byte phase as iq row by row)
__device__ __forceinline__ void iqc_fix_sample(float &re, float &im, float dr, float di, float wr, float wi) {
  if (!iqc_finite(re) || !iqc_finite(im)) return;
  const float zr = __fsub_rn(re, dr), zi = __fsub_rn(im, di);
  re = __fsub_rn(zr, __fadd_rn(__fmul_rn(wr, zr), __fmul_rn(wi, zi)));
  im = __fsub_rn(zi, __fsub_rn(__fmul_rn(wi, zr), __fmul_rn(wr, zi)));
}

__global__ __launch_bounds__(kNbT) void k_iqc_apply(const float2 *__restrict__ iq, long long stride, float2 *__restrict__ out,
                                                    long long ostride, long long n0, long long n1, int pmax,
                                                    const IqcPart *__restrict__ part) {
  const int tid = threadIdx.x, row = blockIdx.y;
  const long long j = n0 / kNbQ + blockIdx.x;
  const long long lo = j * kNbQ > n0 ? j * kNbQ : n0, hi = (j + 1) * kNbQ < n1 ? (j + 1) * kNbQ : n1;
  const long long a = lo - n0, b = hi - n0;
  const float2 *x = iq + (long long)row * stride;
  float2 *o = out + (long long)row * ostride;
  const NbWalk w(x, a);
  nb_v4f v[kNbPairs];
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) v[k] = nb_load_pair(x, w.i0(tid, k), a, b);
  const IqcPart &p = part[(size_t)row * pmax + blockIdx.x];
  const float dr = p.dr, di = p.di, wr = p.wr, wi = p.wi;
  const bool idle = dr == 0.f && di == 0.f && wr == 0.f && wi == 0.f;
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) {
    const long long i0 = w.i0(tid, k);
    const bool in0 = i0 >= a && i0 < b, in1 = i0 + 1 >= a && i0 + 1 < b;
    if (!idle) {
      float r0 = v[k].x, i0v = v[k].y, r1 = v[k].z, i1v = v[k].w;
      iqc_fix_sample(r0, i0v, dr, di, wr, wi);
      iqc_fix_sample(r1, i1v, dr, di, wr, wi);
      v[k].x = r0; v[k].y = i0v; v[k].z = r1; v[k].w = i1v;
    }
    if (in0 && in1) *reinterpret_cast<nb_v4f *>(o + i0) = v[k];
    else if (in0) o[i0] = make_float2(v[k].x, v[k].y);
    else if (in1) o[i0 + 1] = make_float2(v[k].z, v[k].w);
  }
}

// ---- records ----
// one wave per row: the call's pieces in interval order, record by record
__global__ __launch_bounds__(64) void k_iqc_records(const IqcPart *__restrict__ part_all, int pmax, long long n0, long long n1,
                                                    IqcState *__restrict__ state, IqcRec *__restrict__ ring_all, int R, int L) {
  const int lane = threadIdx.x, row = blockIdx.x;
  const IqcPart *part = part_all + (size_t)row * pmax;
  IqcRec *ring = ring_all + (size_t)row * L;
  IqcRec rec = state[row].rec;          // (every lane holds the open record; lane 0 stores it)
  const long long j0 = n0 / kNbQ, j1 = (n1 - 1) / kNbQ;
  long long j = j0;
  while (j <= j1) {
    const long long i = j / R, jend = (i + 1) * R - 1 < j1 ? (i + 1) * R - 1 : j1;      // the intervals j .. jend go to record i
    IqcSum m{};
    unsigned long long nnon = 0, nskip = 0, nref = 0;
    unsigned nint = 0;
    for (long long q = j + lane; q <= jend; q += 64) {
      const IqcPart &p = part[q - j0];
      m.add(p.m);
      nnon += p.nnon; nskip += p.nskip;
      if ((q + 1) * kNbQ <= n1) { nref += p.refused; nint++; }
    }
    for (int d = 32; d > 0; d >>= 1) {
      m.n += __shfl_xor(m.n, d);
#pragma unroll
      for (int q = 0; q < 5; q++) m.s[q] += __shfl_xor(m.s[q], d);
      nnon += __shfl_xor(nnon, d); nskip += __shfl_xor(nskip, d); nref += __shfl_xor(nref, d); nint += __shfl_xor(nint, d);
    }
    rec.index = (uint64_t)i; rec.first_interval = (uint64_t)(i * R);
    rec.n_usable += (uint64_t)m.n; rec.n_nonfinite += nnon; rec.n_skipped += nskip; rec.n_refused += nref;
    rec.sum_re += m.s[0]; rec.sum_im += m.s[1]; rec.sum_rr += m.s[2]; rec.sum_ii += m.s[3]; rec.sum_ri += m.s[4];
    rec.n_intervals += nint;
    const bool last_complete = (jend + 1) * kNbQ <= n1;
    if (last_complete) {
      const IqcPart &p = part[jend - j0];
      rec.dc_re = p.dr; rec.dc_im = p.di; rec.w_re = p.wr; rec.w_im = p.wi;
    }
    if (last_complete && jend == (i + 1) * R - 1) {
      if (lane == 0) ring[i % L] = rec;
      rec = IqcRec{};
    }
    j = jend + 1;
  }
  if (lane == 0) state[row].rec = rec;
}

}  // namespace fmr
