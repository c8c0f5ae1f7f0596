// Channel bank through the facade (host/fmradion_facade.hpp): two FM-stereo stations in one 2.5 MS/s capture, one
// ChannelBank, both channels decoded.  Prints "stereo <ch0> <ch1>" and the audio length; without a GPU the facade stops
// with "no HIP device".
#include <cmath>
#include <cstdio>

#include "fmradion_facade.hpp"

// FM stereo at rate fs, 75 kHz deviation, tones 1000 + 10 id (left) and 400 + 10 id (right) Hz, at +f Hz
static void add_station(IQSampleVector &x, double fs, int id, double amp, long long f) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    const double t = n / fs, th = 2 * M_PI * 19000.0 * t;
    const double l = std::sin(2 * M_PI * (1000.0 + 10 * id) * t), r = std::sin(2 * M_PI * (400.0 + 10 * id) * t);
    ph += 2 * M_PI * 75000.0 / fs * (0.45 * (l + r) + 0.1 * std::sin(th) + 0.45 * (l - r) * std::sin(2 * th));
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

int main() {
  const double fs = 2.5e6;
  IQSampleVector x((size_t)(1.2 * fs));
  add_station(x, fs, 3, 0.3, -600000);
  add_station(x, fs, 8, 0.15, 500000);
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
  std::vector<SampleVector> audio;
  size_t total = 0;
  for (size_t off = 0; off < x.size(); off += 65536) {
    IQSampleVector blk(x.begin() + off, x.begin() + std::min(x.size(), off + 65536));
    bank.process(blk, audio);
    total += audio[0].size();
  }
  std::printf("audio %zu\nstereo %d %d\n", total, (int)bank.stereo_detected(0), (int)bank.stereo_detected(1));
  return bank.stereo_detected(0) && bank.stereo_detected(1) ? 0 : 1;
}
