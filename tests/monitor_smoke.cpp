// Modulation monitor through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz and a two-channel
// ChannelBank at 2.5 MS/s, each station a 1 kHz tone, a pilot and an unmodulated 57 kHz subcarrier at known levels.
// Prints "fm records N pilot P rds R peak K" and "bank0 ..." / "bank1 ..."; exit status 0 when every level is where it
// was put (the 384 kHz decoder is fed the exact inverse of its discriminator; behind the bank's resampler the
// discriminator's own sin(x) / x response shows: 0.4 % at the pilot, 3.6 % at 57 kHz).
#include <cmath>
#include <cstdio>

#include "fmradion_facade.hpp"

static double mpx_at(double t, double pilot) {
  return 0.45 * std::sin(2 * M_PI * 1000.0 * t) + pilot * std::sin(2 * M_PI * 19000.0 * t) +
         (2.0 / 75.0) * std::cos(2 * M_PI * 57000.0 * t);
}

// 75 kHz deviation FM of mpx_at at +f Hz
static void add_station(IQSampleVector &x, double fs, double amp, long long f, double pilot) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * 75000.0 / fs * mpx_at(n / fs, pilot);
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

// response of a phase-difference discriminator at 384 kHz to a component at f Hz of an MPX that reached it band-limited
// (the bank's stations are modulated at 2.5 MS/s and resampled): sin(x) / x, x = pi f / 384000
static double droop(double f) { const double x = M_PI * f / 384000.0; return std::sin(x) / x; }

static bool report(const char *name, const std::vector<ModulationRecord> &recs, size_t want, double pilot, double rds, double tol) {
  if (recs.empty()) { std::printf("%s records 0\n", name); return false; }
  const ModulationRecord &r = recs.back();
  std::printf("%s records %zu pilot %.1f rds %.1f peak %.1f dbr %.2f\n", name, recs.size(), r.levels.pilot_deviation_hz,
              r.levels.rds_deviation_hz, r.levels.peak_deviation_hz, r.levels.mpx_power_dbr);
  bool ok = recs.size() == want;
  for (size_t i = 0; i < recs.size(); i++) ok = ok && recs[i].rec.index == i && recs[i].rec.n_finite == 38400 && recs[i].hist.size() == 64 && recs[i].psd.size() == 513;
  ok = ok && std::fabs(r.levels.pilot_deviation_hz - 75000.0 * pilot) <= tol * 75000.0 * pilot;
  ok = ok && std::fabs(r.levels.rds_deviation_hz - 75000.0 * rds) <= tol * 75000.0 * rds;
  ok = ok && r.levels.peak_deviation_hz > 30000.0 && r.levels.peak_deviation_hz < 45000.0;
  return ok;
}

int main() {
  bool ok = true;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  {
    const double fs = 384000.0;
    IQSampleVector x((size_t)(0.5 * fs));
    add_station(x, fs, 0.3, 0, 0.09);
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_modulation_monitor(38400, 64, 1.0, 8);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 50000)
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 50000)), audio);
    ok = report("fm", fm.read_modulation_records(), (x.size() - 512) / 38400, 0.09, 2.0 / 75.0, 0.01) && ok;
    ok = fm.read_modulation_records().empty() && ok;            // drained
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(0.5 * fs));
    add_station(x, fs, 0.3, -600000, 0.09);
    add_station(x, fs, 0.2, 500000, 0.10);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_modulation_monitor(38400, 64, 1.0, 8);
    std::vector<SampleVector> audio;
    for (size_t off = 0; off < x.size(); off += 65536)
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
    const std::vector<ModulationRecord> r0 = bank.read_modulation_records(0), r1 = bank.read_modulation_records(1);
    ok = report("bank0", r0, r0.size(), 0.09 * droop(19000.0), 2.0 / 75.0 * droop(57000.0), 0.01) && r0.size() >= 4 && ok;
    ok = report("bank1", r1, r0.size(), 0.10 * droop(19000.0), 2.0 / 75.0 * droop(57000.0), 0.01) && ok;
  }
  return ok ? 0 : 1;
}
