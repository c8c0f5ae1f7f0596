// Impulse blanker through the facade (host/fmradion_facade.hpp): FmDecoder, AmDecoder and NbfmDecoder with a front end
// attached, an IfResampler, a two-channel ChannelBank and a Channelizer, all at 2.5 MS/s in FMR_NB_ACT, records of 8
// intervals.  The capture holds two stations with a 1 kHz tone and a burst of two samples at twenty times the carriers
// every 9973 samples behind the first 50000.  Prints "<name> blanked B of N samples in R runs, level L dBFS, peak P dBFS"
// per object; exit status 0 when the records are consecutive and complete, every burst behind the first interval was
// blanked as one run of the default gate's length plus one, the level is the stations', and a second read finds nothing.
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

// a failed check names itself
#define CHECK(cond) ((cond) ? true : (std::printf("failed: %s\n", #cond), false))

constexpr size_t kN = 122 * 4096, kFirst = 50000, kEvery = 9973;
constexpr int kR = 8;

static bool report(const char *name, const BlankerReport &r) {
  if (r.records.empty()) { std::printf("%s records 0\n", name); return false; }
  const fmr_blanker_levels &lv = r.levels;
  std::printf("%s blanked %llu of %llu samples in %llu runs, level %.2f dBFS, peak %.2f dBFS\n", name,
              (unsigned long long)lv.n_blanked, (unsigned long long)lv.n_intervals * 4096, (unsigned long long)lv.n_runs,
              lv.level_dbfs, lv.peak_dbfs);
  bool ok = CHECK(r.records.size() == kN / 4096 / kR && r.info.records_ready == 0 && r.info.records_dropped == 0);
  ok = CHECK(r.info.mode == FMR_NB_ACT && r.info.gate_samples == 2 && r.info.max_run_samples == 16 && r.info.rows == 1) && ok;
  for (size_t i = 0; i < r.records.size(); i++)
    ok = CHECK(r.records[i].index == i && r.records[i].first_interval == i * kR && r.records[i].n_intervals == kR &&
               r.records[i].n_nonfinite == 0) && ok;
  // the bursts inside the complete records: two samples over the threshold, then the gate stays closed one sample more
  unsigned long long bursts = 0;
  for (size_t p = kFirst; p + 3 <= r.records.size() * kR * 4096; p += kEvery) bursts++;
  ok = CHECK(lv.n_runs == bursts && lv.n_triggers == 2 * bursts && lv.n_blanked == 3 * bursts) && ok;
  ok = CHECK(lv.level_dbfs > -9.5 && lv.level_dbfs < -8.0 && lv.peak_dbfs > 14.0 && lv.runs_per_second > 200.0) && ok;
  return ok;
}

template <class Obj, class Out>
static bool run(const char *name, Obj &o, const IQSampleVector &x, Out &out) {
  fmr_blanker_config cfg{};
  cfg.mode = FMR_NB_ACT;
  cfg.record_intervals = kR;
  o.enable_blanker(cfg);
  for (size_t off = 0; off < x.size(); off += 65536)
    o.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), out);
  bool ok = report(name, o.read_blanker());
  return CHECK(o.read_blanker().records.empty()) && ok;    // drained
}

int main() {
  bool ok = true;
  const double fs = 2.5e6;
  IQSampleVector x(kN);
  add_station(x, fs, 0.3, 0, 0.5);
  add_station(x, fs, 0.2, 500000, 0.25);
  for (size_t p = kFirst; p + 2 <= x.size(); p += kEvery) { x[p] += IQSample(6.f, 0.f); x[p + 1] += IQSample(0.f, -6.f); }
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  SampleVector audio;
  {
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.attach_front_end(fs, false);
    ok = run("fm", fm, x, audio) && ok;
  }
  {
    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_am_48khz_narrow");
    AmDecoder am(coeff, ModType::AM);
    am.attach_front_end(fs, false);
    ok = run("am", am, x, audio) && ok;
  }
  {
    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_nbfm_48khz_default");
    NbfmDecoder nb(coeff, NbfmDecoder::freq_dev_normal);
    nb.attach_front_end(fs, false);
    ok = run("nbfm", nb, x, audio) && ok;
  }
  {
    IfResampler ifr(fs, 384000.0);
    IQSampleVector out;
    ok = run("ifr", ifr, x, out) && ok;
  }
  {
    ChannelBank bank(fs, {0, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    std::vector<SampleVector> out;
    ok = run("bank", bank, x, out) && ok;
  }
  {
    Channelizer chz(fs, {0, 500000});
    std::vector<IQSampleVector> out;
    ok = run("channelizer", chz, x, out) && ok;
  }
  return ok ? 0 : 1;
}
