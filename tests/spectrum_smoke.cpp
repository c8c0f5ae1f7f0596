// SpectrumMonitor through the facade (host/fmradion_facade.hpp), then a ChannelBank on the offsets it finds.
//   spectrum_smoke    three FM stations at -1.15 MHz, +0.35 MHz and +2.05 MHz in one 10 MS/s capture; SpectrumMonitor finds
//                     their offsets on the 100 kHz raster offset by 50 kHz, a ChannelBank decodes them.  Prints
//                     "stations <offsets>" and "bank channels 3 audio <n>".  Without a GPU the facade stops with
//                     "no HIP device".
#include <cmath>
#include <cstdio>

#include "fmradion_facade.hpp"

// an FM carrier at rate fs, 75 kHz deviation, a tone of 1000 + 10 id Hz, at +f Hz
static void add_station(IQSampleVector &x, double fs, int id, double amp, long long f) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * 75000.0 / fs * std::sin(2 * M_PI * (1000.0 + 10 * id) * n / fs);
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

int main() {
  const double fs = 10e6;
  const long long want[3] = {-1150000, 350000, 2050000};
  IQSampleVector x(1 << 20);
  for (int k = 0; k < 3; k++) add_station(x, fs, k, 0.1 + 0.05 * k, want[k]);
  SpectrumMonitor mon(fs, 8192);
  mon.process(x);
  fmr_station_rule rule{};
  rule.raster_hz = 100000; rule.raster_offset_hz = 50000; rule.bandwidth_hz = 200000; rule.threshold_db = 10.0;
  const std::vector<int32_t> off = mon.find_stations(rule);
  std::printf("stations");
  for (int32_t f : off) std::printf(" %d", f);
  std::printf("\n");
  if (off.size() != 3) return 1;
  for (int k = 0; k < 3; k++)
    if (off[k] != want[k]) return 1;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  ChannelBank bank(fs, off, ModType::FM, false, delay, true, 50.0, false, 0, FMR_RESAMPLER_FAST);
  std::vector<SampleVector> audio;
  bank.process(x, audio);
  std::printf("bank channels %zu audio %zu\n", bank.channels(), audio[0].size());
  return audio[0].empty() ? 1 : 0;
}
