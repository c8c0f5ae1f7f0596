// SpectrumMonitor's waterfall through the facade (host/fmradion_facade.hpp).
//   waterfall_smoke <file>   a tone that steps up in level over white noise, 40000 samples at 10 MS/s, written to <file> as
//                            raw cf32; a SpectrumMonitor with a waterfall (N = 512, hop 200, 6 segments per line) takes it in
//                            two blocks.  Prints "waterfall <N> <hop> <R> <first_line> <lines>" and, per line,
//                            "line <index> <counted> <N floats in %a>" for the test to compare with the C-ABI's lines.
//                            Without a GPU the facade stops with "no HIP device".
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "fmradion_facade.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const double fs = 10e6;
  const int N = 512, H = 200, R = 6;
  IQSampleVector x(40000);
  uint32_t lcg = 12345u;
  auto rnd = [&lcg]() { lcg = lcg * 1664525u + 1013904223u; return ((lcg >> 8) & 0xffff) / 65536.0 - 0.5; };
  for (size_t n = 0; n < x.size(); n++) {
    const double a = n < x.size() / 2 ? 0.05 : 0.5, ph = 2 * M_PI * 1.2e6 * (double)n / fs;
    x[n] = IQSample((float)(a * std::cos(ph) + 0.02 * rnd()), (float)(a * std::sin(ph) + 0.02 * rnd()));
  }
  FILE *f = std::fopen(argv[1], "wb");
  if (!f || std::fwrite(x.data(), sizeof(IQSample), x.size(), f) != x.size()) return 2;
  std::fclose(f);
  SpectrumMonitor mon(fs, N, H, FMR_WINDOW_HANN, 0, 1 << 15, R, 64);
  mon.process(IQSampleVector(x.begin(), x.begin() + 12345));
  mon.process(IQSampleVector(x.begin() + 12345, x.end()));
  std::vector<float> lines;
  std::vector<uint32_t> counted;
  const uint64_t first = mon.read_waterfall(0, lines, counted);
  std::printf("waterfall %d %d %d %llu %zu\n", N, H, R, (unsigned long long)first, counted.size());
  for (size_t l = 0; l < counted.size(); l++) {
    std::printf("line %llu %u", (unsigned long long)(first + l), counted[l]);
    for (int k = 0; k < N; k++) std::printf(" %a", (double)lines[l * N + k]);
    std::printf("\n");
  }
  return counted.size() >= 3 && lines.size() == counted.size() * (size_t)N ? 0 : 1;
}
