// pll_compose_tree (csrc/pll_compose.hpp, the level-1 up-sweep of the pilot PLL's node pass) on the host: the tree's
// composite of n seeded random contractive affine maps against the sequential chain of the kernels (pll_up_from_lds) and
// against a long-double chain, for the group sizes at which the tree's shape changes.  Both to 1e-12 of the largest
// entry.  Prints one line per size; exit status 0 only if every size passes.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I airspy-fmradion_amd/csrc tests/pll_compose_host.cpp
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pll_compose.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni() {          // splitmix64 -> (-1, 1)
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// [P | q] <- [M P | M q + r], as one step of the kernels' chain: per entry, from r (column 7) or 0, j ascending
template <class T>
static void chain_step(std::vector<T> &pq, const double *map) {
  std::vector<T> out(FMR_MAP);
  for (int i = 0; i < 7; i++)
    for (int k = 0; k < 8; k++) {
      T acc = (k == 7) ? (T)map[i * 8 + 7] : (T)0;
      for (int j = 0; j < 7; j++) {
        if (sizeof(T) == sizeof(double)) acc = (T)std::fma(map[i * 8 + j], (double)pq[j * 8 + k], (double)acc);
        else acc += (T)map[i * 8 + j] * pq[j * 8 + k];
      }
      out[i * 8 + k] = acc;
    }
  pq = out;
}

int main() {
  const int sizes[] = {1, 2, 3, 31, 32};
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
    std::vector<double> seq(FMR_MAP, 0.0);
    std::vector<long double> ref(FMR_MAP, 0.0L);
    for (int i = 0; i < 7; i++) { seq[i * 8 + i] = 1.0; ref[i * 8 + i] = 1.0L; }
    for (int t = 0; t < n; t++) { chain_step(seq, &maps[(size_t)t * FMR_MAP]); chain_step(ref, &maps[(size_t)t * FMR_MAP]); }
    std::vector<double> tree(maps);       // exactly n maps: the sanitizer sees any access past them
    pll_compose_tree<1>(tree.data(), n, 0, [] {});
    double big = 0.0, e_seq = 0.0, e_ref = 0.0;
    for (int e = 0; e < FMR_MAP; e++) {
      big = std::fmax(big, std::fabs((double)ref[e]));
      e_seq = std::fmax(e_seq, std::fabs(tree[e] - seq[e]));
      e_ref = std::fmax(e_ref, (double)fabsl((long double)tree[e] - ref[e]));
    }
    const bool ok = e_seq <= 1e-12 * big && e_ref <= 1e-12 * big && big > 0.0;
    std::printf("n %2d  largest entry %.3e  tree - chain %.3e  tree - long double chain %.3e  %s\n", n, big, e_seq, e_ref,
                ok ? "ok" : "FAIL");
    bad += !ok;
  }
  return bad ? 1 : 0;
}
