// IQ correction through the facade (host/fmradion_facade.hpp): FmDecoder, AmDecoder and NbfmDecoder with a front end
// attached, an IfResampler, a two-channel ChannelBank and a Channelizer, all at 2.5 MS/s in FMR_IQC_ACT with a window of 4
// intervals and records of 8.  The capture holds a strong station at -250 kHz and a weak one at +250 kHz, each with a
// 1 kHz tone, through the receiver model "I exact, Q' = 1.05 (Q cos 3 deg + I sin 3 deg)" with an offset of
// (0.01, -0.006).  Prints "<name> corrected: dc D dBFS, image I dB, gain G dB, phase P deg" per object; exit status 0 when
// the records are consecutive and complete, nothing was skipped or refused, the pooled levels give back the model (gain
// within 0.2 dB, phase within 0.5 degrees, offset within 1e-3: two noise-free tone-modulated carriers are not quite proper
// over 0.2 s, and tests/iqcorr_fixture.py gives 0.083 dB and 0.14 degrees for this capture), and a second read finds
// nothing.
#include <cmath>
#include <cstdio>

#include "fmradion_facade.hpp"

// 75 kHz deviation FM of a 1 kHz tone of MPX amplitude `level` at +f Hz
static void add_station(std::vector<std::complex<double>> &x, double fs, double amp, long long f, double level) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * 75000.0 / fs * level * std::sin(2 * M_PI * 1000.0 * (n / fs));
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += std::complex<double>(amp * std::cos(ph + mix), amp * std::sin(ph + mix));
  }
}

// a failed check names itself
#define CHECK(cond) ((cond) ? true : (std::printf("failed: %s\n", #cond), false))

constexpr size_t kN = 122 * 4096;
constexpr int kR = 8, kW = 4;
constexpr double kGain = 1.05, kPhase = 3.0, kDcRe = 0.01, kDcIm = -0.006;

static bool report(const char *name, const IqCorrectionReport &r) {
  if (r.records.empty()) { std::printf("%s records 0\n", name); return false; }
  const fmr_iq_correction_levels &lv = r.levels;
  std::printf("%s corrected: dc %.2f dBFS, image %.2f dB, gain %.3f dB, phase %.3f deg\n", name, lv.dc_dbfs,
              lv.image_rejection_db, lv.gain_imbalance_db, lv.phase_error_deg);
  bool ok = CHECK(r.records.size() == kN / 4096 / kR && r.info.records_ready == 0 && r.info.records_dropped == 0);
  ok = CHECK(r.info.mode == FMR_IQC_ACT && r.info.correct == (FMR_IQC_DC | FMR_IQC_BALANCE) && r.info.average_intervals == kW &&
             r.info.record_intervals == kR && r.info.rows == 1) && ok;
  for (size_t i = 0; i < r.records.size(); i++)
    ok = CHECK(r.records[i].index == i && r.records[i].first_interval == i * kR && r.records[i].n_intervals == kR &&
               r.records[i].n_usable == kR * 4096 && r.records[i].n_refused == 0 && r.records[i].w_re != 0.f) && ok;
  ok = CHECK(lv.n_skipped == 0 && lv.n_nonfinite == 0 && lv.usable_share == 1.0 && lv.refused == 0) && ok;
  ok = CHECK(std::fabs(lv.gain_imbalance_db - 20 * std::log10(kGain)) < 0.2 && std::fabs(lv.phase_error_deg - kPhase) < 0.5) && ok;
  ok = CHECK(std::fabs(lv.dc_re - kDcRe) < 1e-3 && std::fabs(lv.dc_im - kDcIm) < 1e-3) && ok;
  ok = CHECK(lv.image_rejection_db > 27.0 && lv.image_rejection_db < 31.0) && ok;
  return ok;
}

template <class Obj, class Out>
static bool run(const char *name, Obj &o, const IQSampleVector &x, Out &out) {
  fmr_iq_correction_config cfg{};
  cfg.mode = FMR_IQC_ACT;
  cfg.average_intervals = kW;
  cfg.record_intervals = kR;
  o.enable_iq_correction(cfg);
  for (size_t off = 0; off < x.size(); off += 65536)
    o.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), out);
  bool ok = report(name, o.read_iq_correction());
  return CHECK(o.read_iq_correction().records.empty()) && ok;    // drained
}

int main() {
  bool ok = true;
  const double fs = 2.5e6;
  std::vector<std::complex<double>> s(kN);
  add_station(s, fs, 0.3, -250000, 0.5);
  add_station(s, fs, 0.03, 250000, 0.25);
  IQSampleVector x(kN);
  const double c = std::cos(kPhase * M_PI / 180), sn = std::sin(kPhase * M_PI / 180);
  for (size_t n = 0; n < kN; n++)
    x[n] = IQSample((float)(s[n].real() + kDcRe), (float)(kGain * (s[n].imag() * c + s[n].real() * sn) + kDcIm));
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
    ChannelBank bank(fs, {-250000, 250000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    std::vector<SampleVector> out;
    ok = run("bank", bank, x, out) && ok;
  }
  {
    Channelizer chz(fs, {-250000, 250000});
    std::vector<IQSampleVector> out;
    ok = run("channelizer", chz, x, out) && ok;
  }
  return ok ? 0 : 1;
}
