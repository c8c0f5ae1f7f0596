// RDS through the facade (host/fmradion_facade.hpp): two FM stations with RDS in one 2.5 MS/s capture, one ChannelBank
// with enable_rds(), the PS of both channels.  Prints "ps0 [...]" and "ps1 [...]".
#include <cmath>
#include <cstdio>

#include "fmradion_facade.hpp"

// the biphase doublet of the standard's shaping filter, unit peak (tests/rds_fixture.py: pulse)
static double pulse(double t) {
  const double td = 1.0 / 1187.5, u = 8.0 * t / td;
  if (std::fabs(std::fabs(u) - 1.0) < 1e-9) return M_PI / 4;
  return std::cos(M_PI * u / 2) / (1.0 - u * u);
}

// FM stereo tone + RDS groups 0A carrying `ps` at +f Hz, 75 kHz deviation
static void add_station(IQSampleVector &x, double fs, double amp, long long f, uint16_t pi, const char *ps) {
  std::vector<int> bits;
  for (int rep = 0; rep < 40; rep++)
    for (int seg = 0; seg < 4; seg++) {
      const uint16_t blk[4] = {pi, (uint16_t)(10 << 5 | seg), 0xE0CD, (uint16_t)(ps[2 * seg] << 8 | ps[2 * seg + 1])};
      const uint16_t off[4] = {fmr_rds::kOffsetA, fmr_rds::kOffsetB, fmr_rds::kOffsetC, fmr_rds::kOffsetD};
      for (int b = 0; b < 4; b++) {
        const uint32_t w = (uint32_t)blk[b] << 10 | (fmr_rds::checkword(blk[b]) ^ off[b]);
        for (int i = 25; i >= 0; i--) bits.push_back(w >> i & 1);
      }
    }
  std::vector<double> a(bits.size());
  int e = 0;
  for (size_t k = 0; k < bits.size(); k++) { e ^= bits[k]; a[k] = e ? -1.0 : 1.0; }
  const double td = 1.0 / 1187.5, t0 = 0.002;
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    const double t = n / fs;
    long long k0 = (long long)std::floor((t - t0) / td);
    double m = 0.0;
    for (long long k = k0 - 3; k <= k0 + 4; k++)
      if (k >= 0 && k < (long long)a.size()) {
        const double tk = t0 + k * td;
        m += a[k] * (pulse(t - tk) - pulse(t - tk - td / 2));
      }
    const double mpx = 0.45 * std::sin(2 * M_PI * 1000.0 * t) + 0.1 * std::sin(2 * M_PI * 19000.0 * t) +
                       (2.0 / 75.0) * m * std::sin(2 * M_PI * 57000.0 * t);
    ph += 2 * M_PI * 75000.0 / fs * mpx;
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

int main() {
  const double fs = 2.5e6;
  IQSampleVector x((size_t)(1.5 * fs));
  add_station(x, fs, 0.3, -600000, 0x1A1A, "FACADE A");
  add_station(x, fs, 0.2, 500000, 0x2B2B, "FACADE B");
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
  bank.enable_rds();
  std::vector<SampleVector> audio;
  for (size_t off = 0; off < x.size(); off += 65536) {
    IQSampleVector blk(x.begin() + off, x.begin() + std::min(x.size(), off + 65536));
    bank.process(blk, audio);
  }
  const fmr_rds::Station &s0 = bank.rds_station(0), &s1 = bank.rds_station(1);
  std::printf("ps0 [%s] pi0 %04X\nps1 [%s] pi1 %04X\n", s0.ps.c_str(), s0.pi, s1.ps.c_str(), s1.pi);
  return s0.ps_complete() && s1.ps_complete() && s0.pi == 0x1A1A && s1.pi == 0x2B2B ? 0 : 1;
}
