// The optional stages of a facade decoder survive a chain made anew (host/fmradion_facade.hpp, fmr_detail::Stages):
// FmDecoder and AmDecoder with every stage they offer, each with a configuration that is not the default, through
// attach_front_end() and, for FmDecoder, enable_rds().  After each, every read_*() must find its stage (a read of a
// chain without it throws) with the configured values.
#include <cstdio>
#define FMR_FACADE_THROW
#include "../airspy-fmradion_amd/host/fmradion_facade.hpp"

static bool check(bool ok, const char *expr, const char *where) {
  if (!ok) std::printf("FAILED after %s: %s\n", where, expr);
  return ok;
}
#define CHECK(x) check((x), #x, where)

// the two stages on the capture need a front end: `capture` says whether they have been enabled yet
template <class Dec>
static bool output_analyser_capture(Dec &d, bool capture, const char *where) {
  bool ok = true;
  const OutputData o = d.read_output();
  ok = CHECK(o.info.format == FMR_PCM_F32) && CHECK(d.output_rate_info().rate == 32000) && ok;
  ok = CHECK(d.read_analyser().info.max_records == 13 && d.read_analyser().info.fft_size == 2048) && ok;
  if (capture) {
    ok = CHECK(d.read_blanker().info.max_records == 15 && d.read_blanker().info.mode == FMR_NB_ACT) && ok;
    ok = CHECK(d.read_iq_correction().info.max_records == 17 && d.read_iq_correction().info.average_intervals == 8) && ok;
  }
  return ok;
}

static bool fm_stages(FmDecoder &fm, bool capture, const char *where) {
  bool ok = output_analyser_capture(fm, capture, where);
  fm.read_modulation_records();
  fm.read_rf_records();
  ok = CHECK(fm.read_loudness().info.max_records == 9 && fm.read_loudness().info.step_samples == 480) && ok;
  ok = CHECK(fm.read_weak_signal().info.max_records == 11 && fm.read_weak_signal().info.mode == FMR_WS_ACT) && ok;
  const MpxOutputData m = fm.read_mpx_output();
  return CHECK(m.info.rate == 171000 && m.info.format == FMR_PCM_F32) && ok;
}

template <class Dec>
static void enable_capture_stages(Dec &d) {
  fmr_blanker_config nb{};
  nb.mode = FMR_NB_ACT; nb.max_records = 15;
  d.enable_blanker(nb);
  fmr_iq_correction_config iqc{};
  iqc.average_intervals = 8; iqc.max_records = 17;
  d.enable_iq_correction(iqc);
}

int main() {
  const double fs = 2.5e6;
  bool ok = true;
  try {
    IQSampleCoeff delay{0.f, 1.f, 0.f};
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_modulation_monitor(1024, 64, 0.0, 7);
    fm.enable_loudness(480, 9);
    fmr_weak_signal_config ws{};
    ws.mode = FMR_WS_ACT; ws.max_records = 11;
    fm.enable_weak_signal(ws);
    fm.enable_rf_monitor(1024, 5);
    fm.enable_output(FMR_PCM_F32, 0.0, 0.0, 0, 0, 32000, false);
    fm.enable_analyser(2048, 0, 13);
    fm.enable_mpx_output(FMR_PCM_F32, 171000);
    ok = fm_stages(fm, false, "the enables") && ok;
    fm.attach_front_end(fs, false);
    ok = fm_stages(fm, false, "FmDecoder::attach_front_end") && ok;
    enable_capture_stages(fm);
    fm.attach_front_end(fs, true);
    ok = fm_stages(fm, true, "a second FmDecoder::attach_front_end") && ok;
    fm.enable_rds();
    ok = fm_stages(fm, true, "FmDecoder::enable_rds") && ok;
    // one block: the two monitors' records show their intervals (the defaults, 384000 and 38400 samples, complete none)
    const char *where = "FmDecoder::process";
    SampleVector audio;
    fm.process(IQSampleVector(65536, IQSample(0.3f, 0.0f)), audio);
    const std::vector<ModulationRecord> mod = fm.read_modulation_records();
    ok = CHECK(mod.size() >= 7 && mod[0].hist.size() == 64) && CHECK(!fm.read_rf_records().empty()) && ok;
    std::printf("fm stages kept: %zu audio samples, %zu modulation records\n", audio.size(), mod.size());

    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_am_48khz_narrow");
    AmDecoder am(coeff, ModType::AM);
    am.enable_output(FMR_PCM_F32, 0.0, 0.0, 0, 0, 32000, false);
    am.enable_analyser(2048, 0, 13);
    am.attach_front_end(fs, false);
    ok = output_analyser_capture(am, false, "AmDecoder::attach_front_end") && ok;
    enable_capture_stages(am);
    am.attach_front_end(fs, true);
    ok = output_analyser_capture(am, true, "a second AmDecoder::attach_front_end") && ok;
    std::printf("am stages kept\n");
    return ok ? 0 : 1;
  } catch (const std::exception &e) {
    std::printf("exception: %s\n", e.what());
    return 10;
  }
}
