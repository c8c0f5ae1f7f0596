// Audio monitor through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz and a two-channel ChannelBank at
// 2.5 MS/s.  Each station is mono (no pilot) with a 1 kHz tone at a known deviation, so the audio is L = R at a known
// level.  Prints "fm records N momentary M peak P true T corr C" and "bank0 ..." / "bank1 ..."; exit status 0 when the
// records are consecutive and complete, the loudness is where the tone's level puts it, the true peak is not under the
// sample peak, and the correlation is exactly 1.
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

// A sine of amplitude a in both channels reads 20 log10(a) LUFS at 1 kHz (K-weighting is +0.69 dB there, the standard's
// -0.691 takes it back; two channels of a^2 / 2 each add up to a^2).  The 50 us de-emphasis takes 0.41 dB at 1 kHz.
static bool report(const char *name, const LoudnessReport &r, double level, size_t min_records) {
  if (r.records.empty()) { std::printf("%s records 0\n", name); return false; }
  const fmr_loudness_levels &lv = r.levels;
  std::printf("%s records %zu momentary %.2f integrated %.2f peak %.2f true %.2f corr %.3f silence %llu\n", name, r.records.size(),
              lv.momentary_lufs, lv.integrated_lufs, lv.sample_peak_dbfs, lv.true_peak_dbtp, lv.correlation,
              (unsigned long long)lv.longest_silence_blocks);
  bool ok = r.records.size() >= min_records && r.info.records_ready == 0 && r.info.records_dropped == 0;
  for (size_t i = 0; i < r.records.size(); i++)
    ok = ok && r.records[i].index == i && r.records[i].first_sample == i * 4800 && r.records[i].channels == 2 &&
         r.records[i].step_samples == 4800 && r.records[i].n_nonfinite == 0;
  const double want = 20.0 * std::log10(level) - 0.41;
  ok = ok && std::fabs(lv.momentary_lufs - want) <= 0.5 && std::fabs(lv.integrated_lufs - want) <= 0.5;
  ok = ok && lv.true_peak_dbtp >= lv.sample_peak_dbfs && lv.true_peak_dbtp <= lv.sample_peak_dbfs + 1.0;
  ok = ok && lv.correlation == 1.0 && lv.trailing_silence_blocks == 0;
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
    fm.enable_loudness();
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 50000)
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 50000)), audio);
    ok = report("fm", fm.read_loudness(), 0.5, 9) && ok;
    ok = fm.read_loudness().records.empty() && ok;              // drained
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(1.0 * fs));
    add_station(x, fs, 0.3, -600000, 0.5);
    add_station(x, fs, 0.2, 500000, 0.25);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_loudness();
    std::vector<SampleVector> audio;
    for (size_t off = 0; off < x.size(); off += 65536)
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
    ok = report("bank0", bank.read_loudness(0), 0.5, 9) && ok;
    ok = report("bank1", bank.read_loudness(1), 0.25, 9) && ok;
  }
  return ok ? 0 : 1;
}
