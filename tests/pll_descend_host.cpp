// pll_descend_tree (csrc/pll_compose.hpp, the down-sweep of the pilot PLL's node pass behind a Jacobian round) on the host:
// pll_compose_tree composes n seeded random contractive affine maps and leaves the inner nodes' earlier halves in its sink,
// pll_descend_tree goes down through them from a random start delta.  The delta at the start of every chunk against the
// sequential sweep d[t + 1] = M[t] d[t] + r[t] (per row from r[i], seven fused multiply-adds with j ascending) and against
// the same sweep in long double, for the group sizes at which the tree's shape changes (a slot without a partner, a group of
// one).  Both to 1e-12 of the largest delta, the figure tests/pll_compose_host.cpp holds the up-sweep's tree to: only the
// association differs.  The composite the tree leaves in maps[0] must be what it is without a sink, bit for bit.
// Prints one line per size; exit status 0 only if every size passes.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I airspy-fmradion_amd/csrc tests/pll_descend_host.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pll_compose.hpp"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static double uni() {          // splitmix64 -> (-1, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

template <class T>
static void sweep_step(T (&d)[7], const double *map) {
  T out[7];
  for (int i = 0; i < 7; i++) {
    T acc = (T)map[i * 8 + 7];
    for (int j = 0; j < 7; j++) {
      if (sizeof(T) == sizeof(double)) acc = (T)std::fma(map[i * 8 + j], (double)d[j], (double)acc);
      else acc += (T)map[i * 8 + j] * d[j];
    }
    out[i] = acc;
  }
  for (int i = 0; i < 7; i++) d[i] = out[i];
}

int main() {
  const int sizes[] = {1, 2, 3, 5, 16, 17, 31, 32};
  int bad = 0;
  for (int n : sizes) {
    // contractive: every row's absolute sum is at most 0.9 (infinity norm), offsets of order one
    std::vector<double> maps((size_t)n * FMR_MAP);
    for (int t = 0; t < n; t++)
      for (int i = 0; i < 7; i++) {
        double row[7], sum = 0.0;
        for (int j = 0; j < 7; j++) { row[j] = uni(); sum += std::fabs(row[j]); }
        const double scale = 0.9 * std::fabs(uni()) / sum;
        for (int j = 0; j < 7; j++) maps[(size_t)t * FMR_MAP + i * 8 + j] = row[j] * scale;
        maps[(size_t)t * FMR_MAP + i * 8 + 7] = uni();
      }
    double d0[7];
    for (int i = 0; i < 7; i++) d0[i] = uni();
    // the sequential sweeps: delta at the start of chunk t, t = 0 .. n - 1
    std::vector<double> seq((size_t)n * 7);
    std::vector<long double> ref((size_t)n * 7);
    {
      double d[7]; long double e[7];
      for (int i = 0; i < 7; i++) { d[i] = d0[i]; e[i] = d0[i]; }
      for (int t = 0; t < n; t++) {
        for (int i = 0; i < 7; i++) { seq[(size_t)t * 7 + i] = d[i]; ref[(size_t)t * 7 + i] = e[i]; }
        sweep_step(d, &maps[(size_t)t * FMR_MAP]); sweep_step(e, &maps[(size_t)t * FMR_MAP]);
      }
    }
    // up: exactly n maps and the whole sink (NaN where the tree has nothing to say: the descent must not read there)
    std::vector<double> tree(maps), plain(maps), sink((size_t)FMR_TREE_SINK * FMR_MAP, std::nan(""));
    pll_compose_tree<1>(tree.data(), n, 0, [] {}, sink.data());
    pll_compose_tree<1>(plain.data(), n, 0, [] {});
    const bool same_up = std::memcmp(tree.data(), plain.data(), FMR_MAP * sizeof(double)) == 0;
    // down: the even chunks' own maps (exactly ceil(n / 2)), the even chunks' deltas (exactly ceil(n / 2) x 7)
    const int nev = (n + 1) / 2;
    std::vector<double> leaf((size_t)nev * FMR_MAP), de((size_t)nev * 7, std::nan(""));
    for (int p = 0; p < nev; p++) std::memcpy(&leaf[(size_t)p * FMR_MAP], &maps[(size_t)2 * p * FMR_MAP], FMR_MAP * sizeof(double));
    for (int i = 0; i < 7; i++) de[i] = d0[i];
    pll_descend_tree<1>(sink.data(), leaf.data(), de.data(), n, 0, [] {});
    double big = 0.0, e_seq = 0.0, e_ref = 0.0;
    bool finite = true;
    for (int t = 0; t < n; t++)
      for (int i = 0; i < 7; i++) {
        const double got = pll_descend_delta(leaf.data(), de.data(), t, i);
        finite = finite && std::isfinite(got);
        big = std::fmax(big, std::fabs((double)ref[(size_t)t * 7 + i]));
        e_seq = std::fmax(e_seq, std::fabs(got - seq[(size_t)t * 7 + i]));
        e_ref = std::fmax(e_ref, (double)fabsl((long double)got - ref[(size_t)t * 7 + i]));
      }
    const bool ok = finite && same_up && e_seq <= 1e-12 * big && e_ref <= 1e-12 * big && big > 0.0;
    std::printf("n %2d  largest delta %.3e  descent - sweep %.3e  descent - long double sweep %.3e  composite %s  %s\n", n, big,
                e_seq, e_ref, same_up ? "same" : "DIFFERS", ok ? "ok" : "FAIL");
    bad += !ok;
  }
  return bad ? 1 : 0;
}
