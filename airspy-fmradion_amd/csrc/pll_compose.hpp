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
//
// sink (optional): the composites a later DESCENT through the same tree needs (pll_descend_tree below).  The node of stride s
// at slot a = P s covers chunks a .. a + s - 1; with the start delta d of the node known, its earlier half starts from d and
// its later half from E(d), E = the composite of the earlier half = what slot a holds BEFORE the level of stride s / 2
// composes it away.  That is the result of the level before, for every even pair whose node has a later half: it goes to
// sink[pll_tree_sink_slot(s, P)] from the registers that hold it anyway.  FMR_TREE_SINK maps of FMR_MAP doubles; the
// leaves' earlier halves (s = 2) are the even chunks' own maps and are not stored.
#define FMR_TREE_SINK (FMR_TREE_MAXN / 2 - 1)
FMR_HD inline int pll_tree_sink_slot(int s /* chunks under the node: 4, 8, .. FMR_TREE_MAXN */, int P /* a / s */) {
  return FMR_TREE_MAXN / 2 - 2 * FMR_TREE_MAXN / s + P;
}
template <int NL, class Bar>
FMR_HD inline void pll_compose_tree(double *maps, int n, int lane, Bar &&bar, double *sink = nullptr) {
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
          // the earlier half of the node above, if that node has a later half
          if (sink && !((p0 + p) & 1) && 2 * (p0 + p) * st + 2 * st < n) {
            double *e = sink + (long)pll_tree_sink_slot(4 * st, (p0 + p) >> 1) * FMR_MAP + i * 8 + k0;
#pragma unroll
            for (int q = 0; q < 4; q++) e[q] = res[v][q];
          }
        }
      }
      bar();
    }
  }
}

// The down-sweep of the same group as a descent through that tree: the start delta of every chunk from the start delta of the
// group, in ceil(log2 n) dependent levels instead of n - 1 steps.
//   up:    the sink of pll_compose_tree for this group;
//   leaf:  the maps of the group's EVEN chunks, leaf[p] = map of chunk 2 p (the earlier halves of the lowest level);
//   de:    deltas of the even chunks, de[p * 7 + i] = component i at the start of chunk 2 p; de[0 .. 6] is the group's start
//          delta on entry;
//   the delta at the start of an odd chunk 2 p + 1 goes over the offset column of leaf[p], which only its own task reads
//   (pll_descend_delta reads either).
// A task is one row of one node: r[i], then seven fused multiply-adds with j ascending -- one step of the sequential sweep.
// A node without a later half passes its start delta on unchanged (nothing to do: the earlier half's start is the node's).
// Loop bounds do not depend on n: callers with different n (the two half-waves of the kernel) meet at the same barriers.
// The kernel has room for `up` or `leaf` in its tile, not for both: it stages one behind the other, hence the two halves.
template <int NL, class Bar>
FMR_HD inline void pll_descend_upper(const double *up, double *de, int n, int lane, Bar &&bar) {
  constexpr int PB = NL >= 7 ? NL / 7 : 1;               // nodes per round
  constexpr int TPL = (PB * 7 + NL - 1) / NL;            // tasks per lane and round
  for (int s = FMR_TREE_MAXN; s >= 4; s >>= 1) {         // s chunks under a node, later half at + s / 2
    const int h = s >> 1, nnode = (n + h - 1) / s;       // nodes whose later half exists
#pragma unroll 1
    for (int p0 = 0; p0 < FMR_TREE_MAXN / s; p0 += PB) {
#pragma unroll
      for (int v = 0; v < TPL; v++) {
        const int t = lane * TPL + v, P = p0 + t / 7, i = t - 7 * (t / 7);
        if (t < PB * 7 && P < nnode) {
          const double *row = up + (long)pll_tree_sink_slot(s, P) * FMR_MAP + i * 8;
          const double *d = de + (P * h) * 7;            // chunk P s -> even index P s / 2
          double acc = row[7];
#pragma unroll
          for (int j = 0; j < 7; j++) acc = fma(row[j], d[j], acc);
          de[(P * h + (h >> 1)) * 7 + i] = acc;          // chunk P s + s / 2: no task of this level reads it
        }
      }
      bar();
    }
  }
}
template <int NL, class Bar>
FMR_HD inline void pll_descend_leaves(double *leaf, const double *de, int n, int lane, Bar &&bar) {
  constexpr int PB = NL >= 7 ? NL / 7 : 1;
  constexpr int TPL = (PB * 7 + NL - 1) / NL;
  const int nleaf = n >> 1;                              // odd chunks
#pragma unroll 1
  for (int p0 = 0; p0 < FMR_TREE_MAXN / 2; p0 += PB) {
#pragma unroll
    for (int v = 0; v < TPL; v++) {
      const int t = lane * TPL + v, P = p0 + t / 7, i = t - 7 * (t / 7);
      if (t < PB * 7 && P < nleaf) {
        double *row = leaf + (long)P * FMR_MAP + i * 8;
        const double *d = de + P * 7;
        double acc = row[7];
#pragma unroll
        for (int j = 0; j < 7; j++) acc = fma(row[j], d[j], acc);
        row[7] = acc;
      }
    }
  }
  bar();
}
template <int NL, class Bar>
FMR_HD inline void pll_descend_tree(const double *up, double *leaf, double *de, int n, int lane, Bar &&bar) {
  pll_descend_upper<NL>(up, de, n, lane, bar);
  pll_descend_leaves<NL>(leaf, de, n, lane, bar);
}
// component i of the delta at the start of chunk t of the group, behind pll_descend_tree
FMR_HD inline double pll_descend_delta(const double *leaf, const double *de, int t, int i) {
  return (t & 1) ? leaf[(long)(t >> 1) * FMR_MAP + i * 8 + 7] : de[(t >> 1) * 7 + i];
}
