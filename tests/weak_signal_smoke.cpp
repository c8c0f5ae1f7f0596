// Weak-signal handling through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz in FMR_WS_ACT and a
// two-channel ChannelBank at 2.5 MS/s in FMR_WS_MEASURE.  Each station carries a 1 kHz tone; white noise is added to the
// second half of the FmDecoder's input.  Prints "fm records N usn mean M peak P dB blend share S" and "bank0 ..." /
// "bank1 ..."; exit status 0 when the records are consecutive and complete, the readings are finite, the FmDecoder's
// first records (clean) hold every t at 0 and its last (C/N about 3 dB) at 1, and a second read finds nothing.
#include <cmath>
#include <cstdio>
#include <random>

#include "fmradion_facade.hpp"

// 75 kHz deviation FM of a 1 kHz tone of MPX amplitude `level` at +f Hz
static void add_station(IQSampleVector &x, double fs, double amp, long long f, double level) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * 75000.0 / fs * level * std::sin(2 * M_PI * 1000.0 * (n / fs));
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

// a failed check names itself
#define CHECK(cond) ((cond) ? true : (std::printf("failed: %s\n", #cond), false))

static bool report(const char *name, const WeakSignalReport &r, size_t min_records) {
  if (r.records.empty()) { std::printf("%s records 0\n", name); return false; }
  const fmr_weak_signal_levels &lv = r.levels;
  std::printf("%s records %zu usn mean %.2f peak %.2f dB blend share %.3f last t %.3f %.3f %.3f\n", name, r.records.size(),
              lv.usn_mean_db, lv.usn_peak_db, lv.blend_share, lv.t_blend, lv.t_highcut, lv.t_mute);
  bool ok = CHECK(r.records.size() >= min_records && r.info.records_ready == 0 && r.info.records_dropped == 0);
  for (size_t i = 0; i < r.records.size(); i++) {
    ok = CHECK(r.records[i].index == i && r.records[i].first_interval == i * 50 && r.records[i].n_intervals == 50) && ok;
    ok = CHECK(r.records[i].n_nonfinite == 0 && r.records[i].usn_peak * 50 * (1 + 1e-12) >= r.records[i].usn_sum) && ok;
  }
  ok = CHECK(std::isfinite(lv.usn_mean_db) && lv.usn_peak_db >= lv.usn_mean_db) && ok;
  ok = CHECK(lv.n_intervals == 50 * r.records.size()) && ok;
  return ok;
}

int main() {
  bool ok = true;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  {
    const double fs = 384000.0;
    IQSampleVector x((size_t)(1.0 * fs));
    add_station(x, fs, 0.3, 0, 0.5);
    std::mt19937 rng(3);
    std::normal_distribution<float> g(0.f, 0.15f);
    for (size_t n = x.size() / 2; n < x.size(); n++) x[n] += IQSample(g(rng), g(rng));
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fmr_weak_signal_config cfg{};
    cfg.mode = FMR_WS_ACT;
    fm.enable_weak_signal(cfg);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 50000)
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 50000)), audio);
    const WeakSignalReport r = fm.read_weak_signal();
    ok = report("fm", r, 9) && ok;
    ok = CHECK(r.info.mode == FMR_WS_ACT && r.records.front().max_blend == 0.0 && r.records.front().max_mute == 0.0) && ok;
    ok = CHECK(r.records.back().t_blend == 1.0 && r.records.back().t_highcut == 1.0 && r.records.back().t_mute == 1.0) && ok;
    ok = CHECK(fm.read_weak_signal().records.empty()) && ok;    // drained
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(1.0 * fs));
    add_station(x, fs, 0.3, -600000, 0.5);
    add_station(x, fs, 0.2, 500000, 0.25);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_weak_signal();
    std::vector<SampleVector> audio;
    for (size_t off = 0; off < x.size(); off += 65536)
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
    ok = report("bank0", bank.read_weak_signal(0), 9) && ok;
    ok = report("bank1", bank.read_weak_signal(1), 9) && ok;
  }
  return ok ? 0 : 1;
}
