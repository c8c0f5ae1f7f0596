// kernels_chanbank.hpp -- stage A of the IF resampler for a channel bank (fmr_config.channel_offset_hz).
//
// K channels share one input row x (the capture).  Channel s decodes u_s[n] = x[n] exp(-2 pi i ((f_s n) mod F) / F), and
// stage A of its IF resampler is y_s[m] = sum_k hA[k] u_s[N_m - k] with N_m = D m + ca (absolute sample index).  Since
// exp(-2 pi i f (N - k) / F) = exp(-2 pi i f N / F) exp(+2 pi i f k / F),
//
//     y_s[m] = p_s(N_m) . sum_k c_s[k] x[N_m - k],    c_s[k] = hA[k] exp(+2 pi i ((f_s k) mod F) / F),
//     p_s(N) = exp(-2 pi i ((f_s N) mod F) / F)
//
// ("Channel bank": the modulated-tap form).  The complex taps are built on the host in double precision and
// rounded once to fp32; the rotation p_s is computed per OUTPUT from an exact 64-bit integer phase -- nothing
// accumulates phase in floating point, so the phase is exact for any n a receiver reaches.
//
// One workgroup stages the input span of BLOCK consecutive outputs in LDS once and computes them for a group of
// FMR_CB_G channels: every x sample read from LDS feeds 4 G fp32 FMAs, and the taps of the group ([k][g], wave-uniform)
// come through the scalar cache.  More channels than G are groups along grid.y, each of which stages the span again
// (HBM input bytes per call <= ceil(K / G) x the capture).  fp32 throughout: a non-finite sample poisons exactly the
// outputs whose NA-tap support covers it, in every channel, as the oracle's mix-then-filter does.
// Output layout = the other stage-A kernels': row s of `mid` (stride mid_stride), from column mid_off on.
#pragma once
#include <hip/hip_runtime.h>

#ifndef FMR_CB_G
#define FMR_CB_G 8
#endif

// per channel: f_s mod F, and (f_s mod F) D mod F (the phase step of one output)
struct ChanPhase {
  unsigned long long f, fstep;
};

template <int BLOCK, int G>
__global__ __launch_bounds__(BLOCK) void k_ifr_chan(
    const float2 *__restrict__ iq, long long n_valid, const float2 *__restrict__ halo, int H,
    const float2 *__restrict__ ctaps, int NA, int D, long long top0, int count, float2 *__restrict__ mid,
    long long mid_stride, int mid_off, const ChanPhase *__restrict__ cph, int K, unsigned long long nmod0,
    unsigned long long F) {
  extern __shared__ float2 lds_cb[];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * BLOCK;
  const int span = BLOCK * D + NA - 1;
  const long long lo = top0 + (long long)m0 * D - (NA - 1);
  for (int i = tid; i < span; i += BLOCK) {
    const long long n = lo + i;
    float2 v = make_float2(0.f, 0.f);
    if (n < 0) {
      if (n >= -(long long)H) v = halo[H + n];
    } else if (n < n_valid) {
      v = iq[n];
    }
    lds_cb[i] = v;
  }
  __syncthreads();
  const int m = m0 + tid;
  if (m >= count) return;
  const float2 *xp = lds_cb + tid * D + (NA - 1);
  const float2 *cg = ctaps + (size_t)blockIdx.y * NA * G;
  float ar[G], ai[G];
#pragma unroll
  for (int g = 0; g < G; g++) { ar[g] = 0.f; ai[g] = 0.f; }
#pragma unroll 2
  for (int k = 0; k < NA; k++) {
    const float2 x = xp[-k];
    const float2 *c = cg + (size_t)k * G;
#pragma unroll
    for (int g = 0; g < G; g++) {
      const float2 t = c[g];
      ar[g] = fmaf(t.x, x.x, ar[g]);
      ar[g] = fmaf(-t.y, x.y, ar[g]);
      ai[g] = fmaf(t.x, x.y, ai[g]);
      ai[g] = fmaf(t.y, x.x, ai[g]);
    }
  }
  const int g0 = blockIdx.y * G;
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int ch = g0 + g;
    if (ch >= K) break;
    // (f N_m) mod F = (f (N_0 mod F) + m (f D mod F)) mod F: both terms < 2^64 for F < 2^32, m < 2^32
    const ChanPhase p = cph[ch];
    const unsigned long long ph = ((p.f * nmod0) % F + ((unsigned long long)m * p.fstep) % F) % F;
    double sd, cd;
    sincospi(-2.0 * ((double)ph / (double)F), &sd, &cd);
    const float s = (float)sd, co = (float)cd;
    mid[(long long)ch * mid_stride + mid_off + m] =
        make_float2(fmaf(ar[g], co, -ai[g] * s), fmaf(ar[g], s, ai[g] * co));
  }
}
