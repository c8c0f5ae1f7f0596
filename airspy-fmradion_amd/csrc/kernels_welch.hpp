// kernels_welch.hpp -- the Welch segment engine's device side ("The Welch segment engine"), shared by the band
// spectrum and its waterfall (kernels_spectrum.hpp), the modulation and RF monitors (kernels_monitor.hpp,
// kernels_rfmon.hpp) and the audio analyser (kernels_analyser.hpp).  The host side is welch_plan.hpp.
//
// Indices are absolute, counted from the stream's first sample.  N = FFT size, H = hop, M = samples per record (a multiple
// of H).  Segment j covers the samples [j H, j H + N) and belongs to record floor(j H / M): a record holds spr = M / H
// segments, and its last ones reach into the next record.  A segment belongs to the call that delivers its last sample:
// a call processes the segments it completes and no others, so the cut into calls never changes what a segment holds.
// The samples in front of a call's first one come from the stream's carry ring of the last N samples (sample p at slot
// p mod N: the up to N - 1 samples no complete segment has consumed never collide there), which the reduce kernel of the
// call's last launch refreshes.
//
// Partition.  A record is cut into sb = ceil(spr / sub) aligned sub-blocks of `sub` segments (fixed per chain; the last
// one shorter), numbered g = record * sb + sub-block (welch_sub).  A launch takes the segments [a0, a1) in runs; run r is
// sub-block g0 + r clipped to [a0, a1), so a run never straddles a record boundary, and one workgroup walks it serially
// and writes one partial.  The reduce kernel (one workgroup per stream and record the launch touches: welch_rec) adds a
// record's partials in run order -- fp64, fixed order, no float atomics -- on top of the stream's open record when the
// record began in an earlier launch.  A record whose last segment is in goes to slot (index mod L) of the ring [S][L] --
// unless a later record of the same launch takes that slot --, an open one back to the open record.  The open record
// has two copies by launch parity (read [par], write [par ^ 1]): the block that reads the old copy is not the one that
// writes the new one.  Nothing waits on another workgroup or on the host.
//
// LDS: element e of a transform lives at e + (e >> 5) (one float2 of padding per 32): the radix-4 pass of span 1, whose
// lanes read at a stride of 4 elements, spreads a 32-lane ds_read_b64 group over all 64 banks instead of 16 of them.
#pragma once
#include <hip/hip_runtime.h>

#include "welch_plan.hpp"

namespace fmr {

__device__ __forceinline__ int spec_pad(int e) { return e + (e >> 5); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// The 2^LOGN-point FFT of a workgroup of T threads over the bit-reversed, padded points in lds, tw[i] = exp(-2 pi i i / N):
// one radix-2 pass when LOGN is odd, then radix-4 decimation-in-time passes in place.  Every thread owns whole
// butterflies, one barrier per pass; the output is in natural order, behind a barrier.  k_mon_seg and k_an_seg call it;
// k_spec_seg keeps the same passes written out, because this function inlined there costs its N = 256 waterfall forms six
// VGPRs and with them a wave per SIMD (profiles/welch_engine_codegen.txt).  A change to the passes goes to both.
template <int LOGN, int T>
__device__ __forceinline__ void welch_fft(float2 *lds, const float2 *__restrict__ tw, int tid) {
  constexpr int N = 1 << LOGN;
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
  // length-4 span DFT) -> one length-4 span DFT in natural order; W_{4 span}^{j k} = tw[j k N / (4 span)]
  for (; span < N; span *= 4) {
    const int tstep = N / (4 * span);
#pragma unroll 1                   // (unrolled, k_spec_seg's copy of these passes spills at N = 8192 and 1024 threads)
    for (int q = 0; q < N / 4 / T; q++) {
      const int b = tid + q * T;
      const int jj = b & (span - 1);
      const int base = (b - jj) * 4 + jj;
      const int e0 = spec_pad(base), e1 = spec_pad(base + 2 * span), e2 = spec_pad(base + span), e3 = spec_pad(base + 3 * span);
      const float2 a0 = lds[e0];
      const float2 a1 = cmul(lds[e1], tw[jj * tstep]);
      const float2 a2 = cmul(lds[e2], tw[2 * jj * tstep]);
      const float2 a3 = cmul(lds[e3], tw[3 * jj * tstep]);
      const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
      const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
      // X0 = s02 + s13, X2 = s02 - s13, X1 = d02 - i d13, X3 = d02 + i d13
      lds[e0] = make_float2(s02.x + s13.x, s02.y + s13.y);
      lds[e2] = make_float2(d02.x + d13.y, d02.y - d13.x);
      lds[e1] = make_float2(s02.x - s13.x, s02.y - s13.y);
      lds[e3] = make_float2(d02.x - d13.y, d02.y + d13.x);
    }
    __syncthreads();
  }
}

// What every launch of a record stage carries (MonArgs and AnArgs add their own)
struct WelchArgs {
  long long n0;        // absolute index of the call's first sample
  long long a0, a1;    // the launch takes the segments [a0, a1)
  long long g0;        // sub-block of segment a0
  int spr, sub, sb;    // segments per record, per sub-block, sub-blocks per record = ceil(spr / sub)
};

// The record of reduce block bx (record of segment a0, plus bx) of stream s of S in a launch of `runs` > 0 runs: its
// partials are the rows p_first .. p_first + nsub of the [S][rmax] partials.  carried: it began in an earlier launch (the
// launch's first record only) and starts from the open record at os_in.  done: its last segment is in, and with keep it
// goes to ring slot `slot` (not keep: a later record of the launch takes the slot); not done: to the open record at
// os_out.
struct WelchRec {
  long long l;
  int nsub;
  bool carried, done, keep;
  size_t p_first, os_in, os_out, slot;
};
__device__ __forceinline__ WelchRec welch_rec(const WelchArgs &a, int runs, int rmax, int L, int par, int S, int s, int bx) {
  WelchRec r;
  r.l = a.g0 / a.sb + bx;
  const long long g_last = a.g0 + runs - 1;
  const int b_lo = bx == 0 ? (int)(a.g0 - r.l * a.sb) : 0;
  const int b_hi = (int)(a.sb < g_last - r.l * a.sb + 1 ? a.sb : g_last - r.l * a.sb + 1);
  r.nsub = b_hi - b_lo;
  r.carried = a.a0 > r.l * a.spr;
  const long long last_done = a.a1 / a.spr - 1;     // last record complete after this launch
  r.done = r.l <= last_done;
  r.keep = r.l + L > last_done;
  r.p_first = (size_t)s * rmax + (size_t)(r.l * a.sb + b_lo - a.g0);
  r.os_in = (size_t)par * S + s;
  r.os_out = (size_t)(par ^ 1) * S + s;
  r.slot = (size_t)s * L + (size_t)(r.l % L);
  return r;
}

}  // namespace fmr
