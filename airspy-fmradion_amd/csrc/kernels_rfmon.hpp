// kernels_rfmon.hpp -- RF monitor of the decoder's 384 kHz input (fmr_enable_rf_monitor).
//
// The signal is p[n], the squared magnitude of IF sample n as it enters the decoder, read from the call's IF ring slot
// at the head of the audio tail.  The slot holds one of two forms:
//   IF samples (float2, first at slot + s if_stride + h_if):   p = fl(fl(re re) + fl(im im)), unfused fp32;
//   |x|^2 (float, first at (float *)slot + s 2 if_stride):     p as the front end's discriminator epilogue stored it.
// Everything behind p is the modulation monitor's (kernels_monitor.hpp): absolute indices, N = 1024, H = 512, records
// of M samples cut into aligned sub-blocks, one workgroup per run of segments, the time-domain part over a segment's
// first 512 samples, the windowed radix-4 FFT in LDS, |X|^2 into fp64 registers, one fixed reduction tree per run,
// partials written once and added in run order by the reduce kernel.  The bodies are shared (mon_seg_run,
// mon_reduce_run); what is this file's own is the load of p, the carry of p in front of a call's first sample, and
// the histogram's integer rule:  bin = clamp((bits of p >> 20) - 696, 0, 383), eight bins per octave from 2^-40 to 2^8.
//
// The kernels are kernels_monitor.hpp's k_mon_seg<RfmSrc<NRM>> and k_mon_reduce<RfmSrc<NRM>> (grids (runs, S) and
// (records the launch touches, S); a.bins = kRfmBins, the carry of p at carry + s kMonN).
//
// No sqrt, log or atan on the device; nothing waits on another workgroup or on the host; no float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_monitor.hpp"

namespace fmr {

constexpr int kRfmBins = 384, kRfmBinBase = 696;

// sample i of stream s of the call, from either form of the slot
template <bool NRM>
__device__ __forceinline__ float rfm_p(const void *__restrict__ slot, long long if_stride, int h_if, int s, long long i) {
  if constexpr (NRM) {
    return reinterpret_cast<const float *>(slot)[(long long)s * 2 * if_stride + i];
  } else {
    const float2 v = reinterpret_cast<const float2 *>(slot)[(long long)s * if_stride + h_if + i];
    return v.x * v.x + v.y * v.y;
  }
}

__device__ __forceinline__ int rfm_bin(float p) {
  const int u = (int)(__float_as_uint(p) >> 20) - kRfmBinBase;
  return u < 0 ? 0 : (u > kRfmBins - 1 ? kRfmBins - 1 : u);
}

template <bool NRM>
struct RfmSrc {
  static constexpr int kHist = kRfmBins;
  const void *slot;
  long long if_stride;
  int h_if, s;
  const float *cin;
  long long n0;
  __device__ __forceinline__ static RfmSrc make(const void *slot, long long if_stride, int h_if, int s, const float *cin,
                                                const MonArgs &a) {
    return {slot, if_stride, h_if, s, cin, a.n0};
  }
  __device__ __forceinline__ float fresh(long long i) const { return rfm_p<NRM>(slot, if_stride, h_if, s, i); }
  __device__ __forceinline__ float at(long long p) const {
    return p < n0 ? cin[p & (kMonN - 1)] : rfm_p<NRM>(slot, if_stride, h_if, s, p - n0);
  }
  __device__ __forceinline__ int bin(float v) const { return rfm_bin(v); }
};

}  // namespace fmr
