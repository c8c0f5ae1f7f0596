// Audio analyser through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz, an AmDecoder at 48 kHz and a
// two-channel ChannelBank at 2.5 MS/s.  Each FM station is mono (no pilot) with a 1 kHz tone at a known deviation, so the
// audio is L = R at a known level; the AM station is a carrier modulated 50 % by the same tone.  Prints
// "fm records N tone F Hz L dBFS thd T thd+n U sinad S" and "am ..." / "bank0 ..." / "bank1 ..."; exit status 0 when the
// records are consecutive and complete, the tone is found at 1 kHz, and (FM) its level is where the deviation puts it.
#include <cmath>
#include <cstdio>

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

// level > 0: the tone must read 20 log10(level) - 0.41 dB (the 50 us de-emphasis takes 0.41 dB at 1 kHz) within 0.5 dB
static bool report(const char *name, const AnalyserReport &r, double level, size_t min_records, unsigned ch, unsigned N) {
  if (r.records.empty()) { std::printf("%s records 0\n", name); return false; }
  const fmr_analyser_levels &lv = r.levels;
  std::printf("%s records %zu tone %.3f Hz %.2f dBFS thd %.5f thd+n %.5f sinad %.1f noise %.1f\n", name, r.records.size(),
              lv.tone_hz, lv.tone_dbfs, lv.thd, lv.thd_n, lv.sinad_db, lv.noise_dbfs);
  bool ok = r.records.size() >= min_records && r.info.records_ready == 0 && r.info.records_dropped == 0;
  ok = ok && r.info.fft_size == (int)N && r.info.bins == (int)N / 2 + 1 && r.spectra.size() == r.records.size() * 3 * (N / 2 + 1);
  for (size_t i = 0; i < r.records.size(); i++)
    ok = ok && r.records[i].index == i && r.records[i].first_sample == i * r.info.interval_samples &&
         r.records[i].channels == ch && r.records[i].fft_size == N && r.records[i].skipped == 0 && r.records[i].n_nonfinite == 0;
  ok = ok && lv.tone_found == 1 && std::fabs(lv.tone_hz - 1000.0) < 1.0 && lv.thd < 0.05 && lv.sinad_db > 20.0;
  if (level > 0.0) ok = ok && std::fabs(lv.tone_dbfs - (20.0 * std::log10(level) - 0.41)) <= 0.5;
  return ok;
}

int main() {
  bool ok = true;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  {
    const double fs = 384000.0;
    IQSampleVector x((size_t)(1.0 * fs));
    add_station(x, fs, 0.3, 0, 0.5);
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_analyser(2048, 4096);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 50000)
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 50000)), audio);
    ok = report("fm", fm.read_analyser(), 0.5, 10, 2, 2048) && ok;
    ok = fm.read_analyser().records.empty() && ok;              // drained
  }
  {
    const double fs = 48000.0;
    IQSampleVector x(16 * 2048);
    for (size_t n = 0; n < x.size(); n++) x[n] = IQSample((float)(0.2 * (1.0 + 0.5 * std::sin(2 * M_PI * 1000.0 * n / fs))), 0.f);
    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_am_48khz_narrow");
    AmDecoder am(coeff, ModType::AM);
    am.enable_analyser(1024, 1024);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 2048)
      am.process(IQSampleVector(x.begin() + off, x.begin() + off + 2048), audio);
    AnalyserReport r = am.read_analyser();
    // (the audio AGC is still settling in the first records: judge the last eight)
    if (r.records.size() >= 8) {
      const size_t k = r.records.size() - 8, row = 3 * (size_t)r.info.bins;
      fmr_analyser_rule rule{};
      rule.struct_size = sizeof rule;
      fmr_detail::check(fmr_analyser_derive(r.records.data() + k, r.spectra.data() + k * row, 8, &rule, sizeof rule, &r.levels,
                                            sizeof r.levels), "fmr_analyser_derive");
    }
    ok = report("am", r, 0.0, 20, 1, 1024) && ok;
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(1.0 * fs));
    add_station(x, fs, 0.3, -600000, 0.5);
    add_station(x, fs, 0.2, 500000, 0.25);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_analyser();
    std::vector<SampleVector> audio;
    for (size_t off = 0; off < x.size(); off += 65536)
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
    ok = report("bank0", bank.read_analyser(0), 0.5, 1, 2, 4096) && ok;
    ok = report("bank1", bank.read_analyser(1, 2), 0.25, 1, 2, 4096) && ok;      // (view M: L = R, all of it is in the mid)
  }
  return ok ? 0 : 1;
}
