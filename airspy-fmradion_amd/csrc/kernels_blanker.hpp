// kernels_blanker.hpp -- impulse blanker on the capture, ahead of every front end (fmr_enable_blanker, DESIGN.md
// section 17).  The definitions are in include/fmradion_amd.h; tests/blanker_fixture.py restates them in numpy.
//
// Indices are absolute per input row: sample n counts from the chain's first sample.  Interval j = [j Q, (j + 1) Q),
// Q = 4096.  A call hands in the samples [n0, n1) of every row; a "piece" is the part of one interval inside the call, so
// a call has (n1 - 1) / Q - n0 / Q + 1 pieces and only the first and the last may be short.  Both streaming kernels have
// one workgroup per (piece, row) and read the piece with 16-byte loads (a pair of samples; a row that starts on an odd
// multiple of 8 bytes is walked from the sample in front of it, which is masked out).
//
//   k_nb_level    p = fl32(fl32(re re) + fl32(im im)), q = floor(min(p, 256) 2^36), the 64-bit integer sum over the piece
//                 by a fixed tree, the non-finite count and the largest finite p: one NbPart per piece.
//   k_nb_apply    finishes A of its interval (the piece, on top of the carried open sum for the call's first piece), forms
//                 T of its interval and of the one before from the ring of A (intervals before the call) and the parts
//                 (intervals of the call), stages the trigger bits of its piece and of the G + M samples in front of it
//                 in LDS (in front of the call from the row's carry of trigger bits), and computes gate and blank by
//                 windowed counts on two prefix sums.  It counts triggers, blanked samples and run starts of its piece,
//                 and in FMR_NB_ACT stores the piece, zeroed where blank.  What the next call reads and this launch also
//                 reads -- the open sum and the carry -- exists twice, by call parity: a workgroup reads parity ^ 1 and
//                 writes parity.  The ring slots a launch writes (the call's own intervals) are none of those it reads.
//   k_nb_records  one wave per row, off the front end's path: the parts of the call in interval order into the row's open
//                 record (kept in place: only this wave touches it), a complete record to ring slot (index mod L).
//
// Nothing here waits on another workgroup or on the host, and there are no float atomics (the counts are integers).
// The translation unit is compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmr {

constexpr int kNbQ = 4096;       // samples per interval
constexpr int kNbT = 256;        // threads per workgroup: 8 pairs of samples each
constexpr int kNbPairs = kNbQ / 2 / kNbT + 1;   // pairs per thread: a piece walked from the sample in front has one pair more
constexpr int kNbMaxG = 256, kNbMaxM = 1024, kNbMaxW = 64;
constexpr int kNbHalo = kNbMaxG + kNbMaxM;      // trigger bits in front of a piece: G + M at most
constexpr int kNbE = kNbHalo + kNbQ;            // entries of the LDS arrays at most

// fmr_blanker_record, field for field (the stage checks the size)
struct NbRec {
  uint64_t index, first_interval;
  uint64_t n_triggers, n_blanked, n_nonfinite, n_runs, power_q;
  double threshold;
  uint32_t n_intervals;
  float peak;
};

// one piece: k_nb_level leaves A, nnon and peak, k_nb_apply the rest
struct NbPart {
  unsigned long long A;        // sum of q over the piece
  unsigned long long Afull;    // ... on top of what the interval had before the call
  double T;                    // threshold of the piece's interval
  float peak;
  unsigned nnon, ntrig, nblank, nruns, pad;
};

struct NbCoef {
  int G, M, W, R, L, act;
  double g;                    // 10^(threshold_db / 10)
  double r[kNbMaxW + 1];       // r[c] = 1 / (c 2^48)
};

// what a row carries from call to call besides the ring of A and the trigger carry
struct NbState {
  unsigned long long open[2];  // by call parity: the sum of q of the open interval in front of the next call
  NbRec rec;                   // the open record (k_nb_records alone)
};

typedef float nb_v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float nb_power(float re, float im) { return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)); }
__device__ __forceinline__ bool nb_finite(float p) { return p <= 3.4028234663852886e38f; }      // false for NaN and +Inf (p is never negative)
__device__ __forceinline__ unsigned long long nb_q(float p) {
  return nb_finite(p) ? (unsigned long long)((double)fminf(p, 256.f) * 68719476736.0) : 0ull;
}

// The pairs of a piece.  x is the row at the call's first sample; the piece is the call-relative samples [a, b).  With
// mis = 1 when x sits on an odd multiple of 8 bytes, v = i + mis is even where sample i is 16-byte aligned.  Thread tid's
// k-th pair holds the samples i0 and i0 + 1 with i0 = ((a + mis) & ~1) - mis + 2 (tid + k T); either may lie outside.
struct NbWalk {
  long long first;     // i0 of thread 0's pair 0 (may be a - 1)
  __device__ NbWalk(const float2 *x, long long a) {
    const int mis = (int)(((uintptr_t)x >> 3) & 1);
    first = ((a + mis) & ~1ll) - mis;
  }
  __device__ long long i0(int tid, int k) const { return first + 2 * ((long long)tid + (long long)k * kNbT); }
};

// loads the pair at i0 clipped to [a, b): outside samples come back as 0 (and must be masked by the caller)
__device__ __forceinline__ nb_v4f nb_load_pair(const float2 *x, long long i0, long long a, long long b) {
  nb_v4f v = {0.f, 0.f, 0.f, 0.f};
  if (i0 >= a && i0 + 1 < b) {
    v = *reinterpret_cast<const nb_v4f *>(x + i0);
  } else {
    if (i0 >= a && i0 < b) { const float2 s = x[i0]; v.x = s.x; v.y = s.y; }
    if (i0 + 1 >= a && i0 + 1 < b) { const float2 s = x[i0 + 1]; v.z = s.x; v.w = s.y; }
  }
  return v;
}

// ---- level ----
// iq + row stride: sample n0 of the row.  part[row pmax + piece].
__global__ __launch_bounds__(kNbT) void k_nb_level(const float2 *__restrict__ iq, long long stride, long long n0, long long n1,
                                                   int pmax, NbPart *__restrict__ part) {
  __shared__ unsigned long long r_a[kNbT];
  __shared__ unsigned r_n[kNbT];
  __shared__ float r_p[kNbT];
  const int tid = threadIdx.x, row = blockIdx.y;
  const long long j = n0 / kNbQ + blockIdx.x;
  const long long lo = j * kNbQ > n0 ? j * kNbQ : n0, hi = (j + 1) * kNbQ < n1 ? (j + 1) * kNbQ : n1;
  const long long a = lo - n0, b = hi - n0;
  const float2 *x = iq + (long long)row * stride;
  const NbWalk w(x, a);
  nb_v4f v[kNbPairs];
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) v[k] = nb_load_pair(x, w.i0(tid, k), a, b);
  unsigned long long A = 0;
  unsigned nnon = 0;
  float peak = 0.f;
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) {
    const long long i0 = w.i0(tid, k);
    const float p0 = nb_power(v[k].x, v[k].y), p1 = nb_power(v[k].z, v[k].w);
    if (i0 >= a && i0 < b) {
      if (nb_finite(p0)) { A += nb_q(p0); peak = fmaxf(peak, p0); } else nnon++;
    }
    if (i0 + 1 >= a && i0 + 1 < b) {
      if (nb_finite(p1)) { A += nb_q(p1); peak = fmaxf(peak, p1); } else nnon++;
    }
  }
  r_a[tid] = A; r_n[tid] = nnon; r_p[tid] = peak;
  __syncthreads();
  for (int st = kNbT / 2; st > 0; st >>= 1) {
    if (tid < st) { r_a[tid] += r_a[tid + st]; r_n[tid] += r_n[tid + st]; r_p[tid] = fmaxf(r_p[tid], r_p[tid + st]); }
    __syncthreads();
  }
  if (tid == 0) {
    NbPart &o = part[(size_t)row * pmax + blockIdx.x];
    o.A = r_a[0]; o.nnon = r_n[0]; o.peak = r_p[0];
  }
}

// T_j from the A of the intervals j - c .. j - 1: those before the call's first interval j0 from the ring, the others from
// the call's parts (the first on top of the carried open sum)
__device__ inline double nb_threshold(long long j, long long j0, const unsigned long long *ring, int rmask, const NbPart *part,
                                      unsigned long long open_prev, const NbCoef &cf) {
  if (j <= 0) return __builtin_inf();
  const int c = j < cf.W ? (int)j : cf.W;
  unsigned long long S = 0;
  for (long long i = j - c; i < j; i++) S += i < j0 ? ring[i & rmask] : part[i - j0].A + (i == j0 ? open_prev : 0ull);
  const double t = cf.g * ((double)S * cf.r[c]);
  return t > 9.313225746154785e-10 ? t : 9.313225746154785e-10;       // 2^-30
}

// exclusive prefix sum of the E bytes of src into dst[0 .. E] (dst[E] = the total); tot is kNbT + 1 words of scratch
__device__ inline void nb_scan(const unsigned char *src, unsigned short *dst, int E, unsigned *tot) {
  const int tid = threadIdx.x, K = (E + kNbT - 1) / kNbT;
  const int e0 = tid * K < E ? tid * K : E, e1 = e0 + K < E ? e0 + K : E;
  unsigned s = 0;
  for (int e = e0; e < e1; e++) s += src[e];
  tot[tid] = s;
  __syncthreads();
  for (int st = 1; st < kNbT; st <<= 1) {       // inclusive scan of the threads' totals
    const unsigned add = tid >= st ? tot[tid - st] : 0u;
    __syncthreads();
    tot[tid] += add;
    __syncthreads();
  }
  unsigned run = tot[tid] - s;
  for (int e = e0; e < e1; e++) { dst[e] = (unsigned short)run; run += src[e]; }
  if (tid == kNbT - 1) dst[E] = (unsigned short)tot[kNbT - 1];
  __syncthreads();
}

// ---- apply ----
// iq / stride as above; out / ostride the blanked rows (FMR_NB_ACT; same 16-byte phase as iq row by row).  ring[row
// (rmask + 1) + (j & rmask)]; carry[(par row_count + row) HL + k] = trig of sample n1 - HL + k, HL = G + M.
__global__ __launch_bounds__(kNbT) void k_nb_apply(const float2 *__restrict__ iq, long long stride, float2 *__restrict__ out,
                                                   long long ostride, long long n0, long long n1, int pmax, int par,
                                                   NbPart *__restrict__ part_all, unsigned long long *__restrict__ ring_all,
                                                   int rmask, unsigned char *__restrict__ carry_all, NbState *__restrict__ state,
                                                   NbCoef cf) {
  __shared__ unsigned char s_trig[kNbE], s_gate[kNbE];
  __shared__ unsigned short s_pre[kNbE + 1];
  __shared__ unsigned s_tot[kNbT + 1];
  __shared__ double s_T[2];
  __shared__ unsigned s_cnt[2];
  const int tid = threadIdx.x, row = blockIdx.y, rows = gridDim.y, piece = blockIdx.x;
  const int G = cf.G, M = cf.M, HL = G + M;
  const long long j0 = n0 / kNbQ, j = j0 + piece;
  const long long lo = j * kNbQ > n0 ? j * kNbQ : n0, hi = (j + 1) * kNbQ < n1 ? (j + 1) * kNbQ : n1;
  const long long a = lo - n0, b = hi - n0, N = n1 - n0;
  const int len = (int)(b - a), E = HL + len;
  const float2 *x = iq + (long long)row * stride;
  NbPart *part = part_all + (size_t)row * pmax;
  unsigned long long *ring = ring_all + (size_t)row * (rmask + 1);
  const unsigned char *carry_in = carry_all + ((size_t)(par ^ 1) * rows + row) * HL;
  unsigned char *carry_out = carry_all + ((size_t)par * rows + row) * HL;
  const unsigned long long open_prev = state[row].open[par ^ 1];
  // the piece itself: in flight while the thresholds are formed
  const NbWalk w(x, a);
  nb_v4f v[kNbPairs];
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) v[k] = nb_load_pair(x, w.i0(tid, k), a, b);
  if (tid == 0) { s_T[0] = nb_threshold(j, j0, ring, rmask, part, open_prev, cf); s_cnt[0] = s_cnt[1] = 0; }
  if (tid == 64) s_T[1] = nb_threshold(j - 1, j0, ring, rmask, part, open_prev, cf);
  __syncthreads();
  const double Tj = s_T[0], Tjm1 = s_T[1];
  // trigger bits: entry e stands for the call-relative sample a - HL + e
  for (int e = tid; e < HL; e += kNbT) {
    const long long i = a - HL + e;
    unsigned char t = 0;
    if (i < 0) {
      t = carry_in[HL + i];                                  // (i >= -HL; samples in front of the chain's first are 0)
    } else {
      const float2 s = x[i];
      const float p = nb_power(s.x, s.y);
      t = !nb_finite(p) || (double)p > ((n0 + i) / kNbQ == j ? Tj : Tjm1);
    }
    s_trig[e] = t;
  }
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) {
    const long long i0 = w.i0(tid, k);
    const float p0 = nb_power(v[k].x, v[k].y), p1 = nb_power(v[k].z, v[k].w);
    if (i0 >= a && i0 < b) s_trig[HL + (int)(i0 - a)] = !nb_finite(p0) || (double)p0 > Tj;
    if (i0 + 1 >= a && i0 + 1 < b) s_trig[HL + (int)(i0 + 1 - a)] = !nb_finite(p1) || (double)p1 > Tj;
  }
  __syncthreads();
  // gate[e] = a trigger among e - G + 1 .. e (valid from e = G - 1 on)
  nb_scan(s_trig, s_pre, E, s_tot);
  const unsigned ntrig = (unsigned)s_pre[E] - (unsigned)s_pre[HL];
  for (int e = tid; e < E; e += kNbT) s_gate[e] = e >= G - 1 && s_pre[e + 1] != s_pre[e - G + 1];
  __syncthreads();
  // blank[e] = gate[e] and a sample among e - M .. e - 1 that lies in front of the chain's first or has an open gate
  nb_scan(s_gate, s_pre, E, s_tot);
  auto blank = [&](int e) -> bool {            // e >= HL - 1
    if (!s_gate[e]) return false;
    const long long n = n0 + a - HL + e;
    return n < M || (int)s_pre[e] - (int)s_pre[e - M] < M;
  };
  unsigned nblank = 0, nruns = 0;
#pragma unroll
  for (int k = 0; k < kNbPairs; k++) {
    const long long i0 = w.i0(tid, k);
    const bool in0 = i0 >= a && i0 < b, in1 = i0 + 1 >= a && i0 + 1 < b;
    const int e = HL + (int)(i0 - a);
    // (entries from HL - 1 on are valid, and sample i0 of a pair whose second sample is the piece's first sits at HL - 1;
    // in front of the chain's first sample nothing is blanked: the carry starts as zeros)
    const bool prev0 = in0 && blank(e - 1), b0 = in0 && blank(e);
    const bool prev1 = in1 && blank(e), b1 = in1 && blank(e + 1);
    nblank += (unsigned)b0 + (unsigned)b1;
    nruns += (unsigned)(b0 && !prev0) + (unsigned)(b1 && !prev1);
    if (cf.act) {
      if (b0) { v[k].x = 0.f; v[k].y = 0.f; }
      if (b1) { v[k].z = 0.f; v[k].w = 0.f; }
      float2 *o = out + (long long)row * ostride;      // plain stores: the front end reads these rows next (a non-temporal hint measured the same)
      if (in0 && in1) *reinterpret_cast<nb_v4f *>(o + i0) = v[k];
      else if (in0) o[i0] = make_float2(v[k].x, v[k].y);
      else if (in1) o[i0 + 1] = make_float2(v[k].z, v[k].w);
    }
  }
  if (nblank) atomicAdd(&s_cnt[0], nblank);
  if (nruns) atomicAdd(&s_cnt[1], nruns);
  // the carry of the next call: trig of the samples N - HL .. N - 1
  for (int k = tid; k < HL; k += kNbT) {
    const long long i = N - HL + k;
    if (i >= a && i < b) carry_out[k] = s_trig[HL + (int)(i - a)];
    else if (i < 0 && piece == 0) carry_out[k] = carry_in[k + N];     // (a call shorter than the carry: k + N < HL)
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned long long Afull = part[piece].A + (piece == 0 ? open_prev : 0ull);
    const bool complete = (j + 1) * kNbQ <= n1;
    part[piece].Afull = Afull; part[piece].T = Tj;
    part[piece].ntrig = ntrig; part[piece].nblank = s_cnt[0]; part[piece].nruns = s_cnt[1];
    if (complete) ring[j & rmask] = Afull;
    if (hi == n1) state[row].open[par] = complete ? 0ull : Afull;
  }
}

// ---- records ----
// one wave per row: the call's pieces in interval order, record by record
__global__ __launch_bounds__(64) void k_nb_records(const NbPart *__restrict__ part_all, int pmax, long long n0, long long n1,
                                                   NbState *__restrict__ state, NbRec *__restrict__ ring_all, int R, int L) {
  const int lane = threadIdx.x, row = blockIdx.x;
  const NbPart *part = part_all + (size_t)row * pmax;
  NbRec *ring = ring_all + (size_t)row * L;
  NbRec rec = state[row].rec;           // (every lane holds the open record; lane 0 stores it)
  const long long j0 = n0 / kNbQ, j1 = (n1 - 1) / kNbQ;
  long long j = j0;
  while (j <= j1) {
    const long long i = j / R, jend = (i + 1) * R - 1 < j1 ? (i + 1) * R - 1 : j1;      // the intervals j .. jend go to record i
    unsigned long long ntrig = 0, nblank = 0, nnon = 0, nruns = 0, pq = 0;
    unsigned nint = 0;
    float peak = 0.f;
    for (long long q = j + lane; q <= jend; q += 64) {
      const NbPart p = part[q - j0];
      ntrig += p.ntrig; nblank += p.nblank; nnon += p.nnon; nruns += p.nruns;
      peak = fmaxf(peak, p.peak);
      if ((q + 1) * kNbQ <= n1) { pq += p.Afull >> 12; nint++; }
    }
    for (int d = 32; d > 0; d >>= 1) {
      ntrig += __shfl_xor(ntrig, d); nblank += __shfl_xor(nblank, d); nnon += __shfl_xor(nnon, d);
      nruns += __shfl_xor(nruns, d); pq += __shfl_xor(pq, d); nint += __shfl_xor(nint, d);
      peak = fmaxf(peak, __shfl_xor(peak, d));
    }
    rec.index = (uint64_t)i; rec.first_interval = (uint64_t)(i * R);
    rec.n_triggers += ntrig; rec.n_blanked += nblank; rec.n_nonfinite += nnon; rec.n_runs += nruns; rec.power_q += pq;
    rec.n_intervals += nint; rec.peak = fmaxf(rec.peak, peak);
    const bool last_complete = (jend + 1) * kNbQ <= n1;
    if (last_complete) rec.threshold = part[jend - j0].T;
    if (last_complete && jend == (i + 1) * R - 1) {
      if (lane == 0) ring[i % L] = rec;
      rec = NbRec{};
    }
    j = jend + 1;
  }
  if (lane == 0) state[row].rec = rec;
}

}  // namespace fmr
