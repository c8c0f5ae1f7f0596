// RF monitor through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz fed a carrier of amplitude 0.3
// with 10 % AM at 3 kHz on its envelope, and a two-channel ChannelBank at 2.5 MS/s with stations of amplitude 0.3 and 0.2.
// Prints "fm records N level L cn C am_audio A" and "bank0 ..." / "bank1 ..."; exit status 0 when every level is where it
// was put: the level at 20 log10(amplitude) (+ the AM's own m^2 / 2), the envelope AM at
// 10 log10((2 m^2 + m^4 / 8) / (4 (1 + m^2 / 2)^2)) = -23.05 dB, none on the bank's clean stations.
#include <cmath>
#include <cstdio>

#include "fmradion_facade.hpp"

// 75 kHz deviation FM of a 1 kHz tone at +f Hz, envelope amp (1 + m sin 2 pi 3000 t)
static void add_station(IQSampleVector &x, double fs, double amp, long long f, double m) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * 75000.0 / fs * 0.45 * std::sin(2 * M_PI * 1000.0 * (n / fs));
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    const double a = amp * (1.0 + m * std::sin(2 * M_PI * 3000.0 * (n / fs)));
    x[n] += IQSample((float)(a * std::cos(ph + mix)), (float)(a * std::sin(ph + mix)));
  }
}

static bool report(const char *name, const std::vector<RfRecord> &recs, size_t want, double level_db, double tol_db) {
  if (recs.empty()) { std::printf("%s records 0\n", name); return false; }
  const RfRecord &r = recs.back();
  std::printf("%s records %zu level %.2f cn %.1f am_audio %.2f am_rms %.4f p10 %.2f\n", name, recs.size(), r.levels.level_dbfs,
              r.levels.cn_db, r.levels.am_audio_db, r.levels.am_rms, r.levels.p10_dbfs);
  bool ok = recs.size() == want;
  for (size_t i = 0; i < recs.size(); i++)
    ok = ok && recs[i].rec.index == i && recs[i].rec.n_finite == 38400 && recs[i].hist.size() == FMR_RF_HIST_BINS &&
         recs[i].psd.size() == FMR_RF_PSD_BINS && recs[i].rec.segments == 75;
  ok = ok && std::fabs(r.levels.level_dbfs - level_db) <= tol_db;
  ok = ok && r.levels.p10_dbfs <= r.levels.p50_dbfs && r.levels.p50_dbfs <= r.levels.p90_dbfs && r.levels.p90_dbfs <= r.levels.level_dbfs + 1.0;
  return ok;
}

int main() {
  bool ok = true;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  {
    const double fs = 384000.0, m = 0.1;
    IQSampleVector x((size_t)(0.5 * fs));
    add_station(x, fs, 0.3, 0, m);
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_rf_monitor(38400, 8);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 50000)
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 50000)), audio);
    const std::vector<RfRecord> r = fm.read_rf_records();
    ok = report("fm", r, (x.size() - 512) / 38400, 10.0 * std::log10(0.09 * (1.0 + m * m / 2)), 0.01) && ok;
    const double am = 10.0 * std::log10((2 * m * m + m * m * m * m / 8) / (4 * (1 + m * m / 2) * (1 + m * m / 2)));
    ok = !r.empty() && std::fabs(r.back().levels.am_audio_db - am) <= 0.01 && ok;
    ok = fm.read_rf_records().empty() && ok;            // drained
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(0.5 * fs));
    add_station(x, fs, 0.3, -600000, 0.0);
    add_station(x, fs, 0.2, 500000, 0.0);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_rf_monitor(38400, 8);
    std::vector<SampleVector> audio;
    for (size_t off = 0; off < x.size(); off += 65536)
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
    const std::vector<RfRecord> r0 = bank.read_rf_records(0), r1 = bank.read_rf_records(1);
    ok = report("bank0", r0, r0.size(), 20.0 * std::log10(0.3), 0.5) && r0.size() >= 4 && ok;
    ok = report("bank1", r1, r0.size(), 20.0 * std::log10(0.2), 0.5) && ok;
    ok = !r0.empty() && !r1.empty() && r0.back().levels.am_audio_db < -40.0 && r1.back().levels.am_audio_db < -40.0 && ok;
  }
  return ok ? 0 : 1;
}
