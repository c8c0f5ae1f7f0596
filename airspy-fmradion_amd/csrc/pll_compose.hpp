// Composition of the pilot PLL's affine chunk maps as a balanced tree (the node pass's up-sweep, kernels_par.hpp).
// Plain C++ apart from the two function attributes: tests/pll_compose_host.cpp compiles it with the host compiler.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FMR_HD __host__ __device__
#else
#define FMR_HD
#endif

#define FMR_MAP 56            // doubles per map: 7 rows of [M[i][0..6] | r[i]], the layout of PQ / PRE
#define FMR_TREE_MAXN 32      // maps per call at most (FMR_NODE_GRP, FMR_NODE_GRP2)

// maps[t] (t = 0 .. n-1, in time order) are affine maps d -> M d + r.  Leaves their composite
// maps[n-1] o ... o maps[0] in maps[0]; the other slots hold partial composites afterwards.
//   level with stride st: slot a = 2 p st takes  maps[a + st] o maps[a]  = [M_b M_a | M_b r_a + r_b]  for every pair whose
//   later half exists; a slot without a partner stands as it is.  ceil(log2 n) levels, in time order within each pair.
// NL lanes share a level: a task is four neighbouring entries of one output row (fourteen tasks per pair), every entry
// a chain of seven fused multiply-adds of its own -- the same chain, from the same start value, as one step of the
// sequential sweep (pll_up_from_lds), so only the association differs.  The composite goes over the pair's earlier
// slot, which only the pair's own tasks read: they all run in one round (NL / 14 pairs a round), keep their results in
// registers until every lane has read its operands (bar()), then write.  No second buffer, nothing held across rounds.
// NL = 64, bar = the workgroup barrier in the kernel; NL = 1, bar = nothing on the host.
template <int NL, class Bar>
FMR_HD inline void pll_compose_tree(double *maps, int n, int lane, Bar &&bar) {
  constexpr int PB = NL >= 14 ? NL / 14 : 1;             // pairs per round
  constexpr int TPL = (PB * 14 + NL - 1) / NL;           // tasks per lane and round
  for (int st = 1; st < n; st <<= 1) {
    const int npair = (n + st - 1) / (2 * st);
#pragma unroll 1
    for (int p0 = 0; p0 < npair; p0 += PB) {
      const int ntask = (npair - p0 < PB ? npair - p0 : PB) * 14;
      double res[TPL][4];
#pragma unroll
      for (int v = 0; v < TPL; v++) {
        const int t = lane * TPL + v;
        if (t < ntask) {
          const int p = t / 14, u = t - 14 * p, i = u >> 1, k0 = (u & 1) * 4;
          const double *A = maps + (long)(2 * (p0 + p) * st) * FMR_MAP, *B = A + (long)st * FMR_MAP;   // A: the earlier
          const double *brow = B + i * 8;
          double acc[4] = {0.0, 0.0, 0.0, k0 ? brow[7] : 0.0};
#pragma unroll
          for (int j = 0; j < 7; j++)
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q] = fma(brow[j], A[j * 8 + k0 + q], acc[q]);
#pragma unroll
          for (int q = 0; q < 4; q++) res[v][q] = acc[q];
        }
      }
      bar();
#pragma unroll
      for (int v = 0; v < TPL; v++) {
        const int t = lane * TPL + v;
        if (t < ntask) {
          const int p = t / 14, u = t - 14 * p, i = u >> 1, k0 = (u & 1) * 4;
          double *o = maps + (long)(2 * (p0 + p) * st) * FMR_MAP + i * 8 + k0;
#pragma unroll
          for (int q = 0; q < 4; q++) o[q] = res[v][q];
        }
      }
      bar();
    }
  }
}
