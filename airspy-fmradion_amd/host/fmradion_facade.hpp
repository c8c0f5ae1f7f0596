// fmradion_facade.hpp -- C++ facade above the C-ABI (include/fmradion_amd.h) with
// the reference's class names, constructor arguments and member signatures, so
// that the reference's stream loop (main.cpp:879-1002) compiles against it
// unchanged:
//
//   FourthConverterIQ   include/FourthConverterIQ.h:30-82
//   IfResampler         include/IfResampler.h:28-44
//   FmDecoder           include/FmDecode.h:35-164
//   AmDecoder           include/AmDecode.h:33-103
//   NbfmDecoder         include/NbfmDecode.h:30-95
//   FilterParameters    include/FilterParameters.h:29-53
//   ChannelBank         several decoders over one wideband capture (no reference counterpart)
//   Channelizer         several IfResamplers over one wideband capture (no reference counterpart)
//   SpectrumMonitor     band spectrum of a capture and the stations in it (no reference counterpart)
//
// Header-only; link with libfmradion_amd.so.  Every process() call is one
// fmr_process()/fmr_resample() on a one-stream chain (host buffers in, host
// buffers out); the batched device-resident entry points of the C-ABI are what
// bench.py and multi-stream users call directly.
//
// Differences a maintainer has to know (all stated in DESIGN.md):
//  * FourthConverterIQ + IfResampler + decoder can be fused into ONE chain
//    (FmDecoder::attach_front_end) so that the IF samples never leave HBM; used
//    separately they behave like the reference classes (IF samples round-trip
//    through host vectors, as in main.cpp).
//  * IfResampler / AudioResampler arithmetic is this project's resampler
//    specification, not r8brain's (absent from the reference tree).
//  * Errors: the reference classes cannot fail and throw nothing.  A failing HIP call here is fatal in the way
//    main.cpp treats its own fatal errors (message on stderr, exit(1), main.cpp:764-767); define
//    FMR_FACADE_THROW before including this header to get std::runtime_error instead (the tests do).
#pragma once
#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fmradion_amd.h"
#include "fmradion_rds.hpp"

using IQSample = std::complex<float>;
using IQSampleVector = std::vector<IQSample>;
using IQSampleDecodedVector = std::vector<float>;
using Sample = double;
using SampleVector = std::vector<Sample>;
using IQSampleCoeff = std::vector<IQSample::value_type>;
using SampleCoeff = std::vector<SampleVector::value_type>;
enum class ModType { FM, NBFM, AM, DSB, USB, LSB, CW, WSPR };   // include/SoftFM.h:49

namespace fmr_detail {
inline void check(int rc, const char *what) {
  if (rc == FMR_OK) return;
#ifdef FMR_FACADE_THROW
  throw std::runtime_error(std::string(what) + ": " + fmr_last_error());
#else
  std::fprintf(stderr, "ERROR: %s: %s\n", what, fmr_last_error());
  std::exit(1);
#endif
}
inline void fail(const char *what) {
#ifdef FMR_FACADE_THROW
  throw std::runtime_error(what);
#else
  std::fprintf(stderr, "ERROR: %s\n", what);
  std::exit(1);
#endif
}
inline fmr_chain *make(const fmr_config &cfg0, bool rds = false) {
  fmr_config cfg = cfg0;
  cfg.struct_size = sizeof(fmr_config);      // the header this translation unit was built against
  cfg.in_order = 1;                          // every facade call goes through host buffers and synchronises: nothing for the
                                             // pipelined chain to overlap (include/fmradion_amd.h)
  fmr_chain *c = nullptr;
  if (rds) check(fmr_create_rds(&cfg, sizeof cfg, &c), "fmr_create_rds");
  else check(fmr_create(&cfg, &c), "fmr_create");
  return c;
}
inline void rds_correction(fmr_chain *c, int mode, int max_burst, int soft_symbols, double soft_max_cost) {
  fmr_rds_fec fec{};
  fec.struct_size = sizeof fec;
  fec.mode = mode; fec.max_burst = max_burst; fec.soft_symbols = soft_symbols; fec.soft_max_cost = soft_max_cost;
  check(fmr_set_rds_correction(c, &fec, sizeof fec), "fmr_set_rds_correction");
}

// the RDS groups of one stream decoded so far (drained from its queue), also collected into `station`
inline std::vector<fmr_rds_group> rds_groups(fmr_chain *c, int stream, fmr_rds::Station &station) {
  std::vector<fmr_rds_group> out;
  fmr_rds_group buf[256];
  for (int n; (n = fmr_get_rds_groups(c, stream, buf, 256)) > 0;) out.insert(out.end(), buf, buf + n);
  for (const auto &g : out) station.add(g);
  return out;
}

// One drained record of the modulation monitor (fmr_monitor_*: histogram of hist_bins counters, one-sided PSD of the MPX,
// 513 bins of 375 Hz) or of the RF monitor (fmr_rf_monitor_*: 384 bins, eight per octave of power; the PSD of |x|^2), with
// the levels derived from it alone
template <class Rec, class Levels>
struct MonitorRecord {
  Rec rec{};
  std::vector<uint32_t> hist;
  std::vector<double> psd;
  Levels levels{};
};
using ModulationRecord = MonitorRecord<fmr_monitor_record, fmr_monitor_levels>;
using RfRecord = MonitorRecord<fmr_rf_monitor_record, fmr_rf_monitor_levels>;
// ... and all that wait, oldest first, record by record: read(rec, hist, psd, cap, info) and derive(r) are the monitor's
// C functions
template <class R, class Info, class Read, class Derive>
std::vector<R> monitor_drain(const char *read_name, const char *derive_name, Read &&read, Derive &&derive) {
  Info info{};
  const int ready = read(nullptr, nullptr, nullptr, 0, &info);
  if (ready < 0) check(ready, read_name);
  std::vector<R> out;
  for (int i = 0; i < ready; i++) {
    R r;
    r.hist.resize((size_t)info.hist_bins);
    r.psd.resize((size_t)info.psd_bins);
    const int n = read(&r.rec, r.hist.data(), r.psd.data(), 1, nullptr);
    if (n < 0) check(n, read_name);
    if (n == 0) break;
    r.levels.struct_size = sizeof r.levels;
    check(derive(r), derive_name);
    out.push_back(std::move(r));
  }
  return out;
}
inline std::vector<ModulationRecord> monitor_records(fmr_chain *c, int stream) {
  return monitor_drain<ModulationRecord, fmr_monitor_info>(
      "fmr_monitor_read", "fmr_monitor_derive",
      [&](fmr_monitor_record *rec, uint32_t *hist, double *psd, int cap, fmr_monitor_info *info) {
        return fmr_monitor_read(c, stream, rec, hist, psd, cap, info, info ? sizeof *info : 0);
      },
      [](ModulationRecord &r) { return fmr_monitor_derive(&r.rec, r.psd.data(), 1, &r.levels, sizeof r.levels); });
}
inline std::vector<RfRecord> rf_records(fmr_chain *c, int stream) {
  return monitor_drain<RfRecord, fmr_rf_monitor_info>(
      "fmr_rf_monitor_read", "fmr_rf_monitor_derive",
      [&](fmr_rf_monitor_record *rec, uint32_t *hist, double *psd, int cap, fmr_rf_monitor_info *info) {
        return fmr_rf_monitor_read(c, stream, rec, hist, psd, cap, info, info ? sizeof *info : 0);
      },
      [](RfRecord &r) { return fmr_rf_monitor_derive(&r.rec, r.hist.data(), r.psd.data(), 1, &r.levels, sizeof r.levels); });
}

// What waits on one stream (or input row) of a stage whose records are pooled: the drained records in ascending order and
// the levels derived from them together.  The audio monitor (fmr_loudness_*), weak-signal handling (fmr_weak_signal_*),
// the impulse blanker (fmr_blanker_*) and the DC-offset and IQ-imbalance correction (fmr_iq_correction_*) report so.
template <class Rec, class Info, class Levels>
struct Report {
  std::vector<Rec> records;
  Info info{};
  Levels levels{};      // (of `records`; all zero when there are none)
};
using LoudnessReport = Report<fmr_loudness_record, fmr_loudness_info, fmr_loudness_levels>;
using WeakSignalReport = Report<fmr_weak_signal_record, fmr_weak_signal_info, fmr_weak_signal_levels>;
using BlankerReport = Report<fmr_blanker_record, fmr_blanker_info, fmr_blanker_levels>;
using IqCorrectionReport = Report<fmr_iq_correction_record, fmr_iq_correction_info, fmr_iq_correction_levels>;
// count (cap = 0), size, read, derive: read(recs, cap, info, info_size) and derive(recs, n, levels, levels_size) are the
// stage's C functions
template <class R, class Read, class Derive>
R report(const char *read_name, const char *derive_name, Read &&read, Derive &&derive) {
  R out;
  const int ready = read(nullptr, 0, &out.info, sizeof out.info);
  if (ready < 0) check(ready, read_name);
  if (ready == 0) return out;
  out.records.resize((size_t)ready);
  const int n = read(out.records.data(), ready, &out.info, sizeof out.info);
  if (n < 0) check(n, read_name);
  out.records.resize((size_t)n);
  if (n > 0) check(derive(out.records.data(), n, &out.levels, sizeof out.levels), derive_name);
  return out;
}
inline LoudnessReport loudness_report(fmr_chain *c, int stream, double silence_dbfs) {
  return report<LoudnessReport>(
      "fmr_loudness_read", "fmr_loudness_derive", [&](auto... a) { return fmr_loudness_read(c, stream, a...); },
      [&](const fmr_loudness_record *r, int n, auto... a) { return fmr_loudness_derive(r, n, silence_dbfs, a...); });
}
inline WeakSignalReport weak_signal_report(fmr_chain *c, int stream) {
  return report<WeakSignalReport>("fmr_weak_signal_read", "fmr_weak_signal_derive",
                                  [&](auto... a) { return fmr_weak_signal_read(c, stream, a...); },
                                  [](auto... a) { return fmr_weak_signal_derive(a...); });
}
inline BlankerReport blanker_report(fmr_chain *c, int row, double input_rate) {
  return report<BlankerReport>(
      "fmr_blanker_read", "fmr_blanker_derive", [&](auto... a) { return fmr_blanker_read(c, row, a...); },
      [&](const fmr_blanker_record *r, int n, auto... a) { return fmr_blanker_derive(r, n, input_rate, a...); });
}
inline IqCorrectionReport iq_correction_report(fmr_chain *c, int row) {
  return report<IqCorrectionReport>("fmr_iq_correction_read", "fmr_iq_correction_derive",
                                    [&](auto... a) { return fmr_iq_correction_read(c, row, a...); },
                                    [](auto... a) { return fmr_iq_correction_derive(a...); });
}

// audio analyser (fmr_enable_analyser / fmr_analyser_read / fmr_analyser_derive): the drained records in ascending order
// with their spectra [n][3][bins] (scaled to power), and the levels of all of them pooled under `rule`
struct AnalyserReport {
  std::vector<fmr_analyser_record> records;
  std::vector<double> spectra;
  fmr_analyser_info info{};
  fmr_analyser_levels levels{};      // (of `records`; all zero when there are none)
};
// (one read, sized by the ring of cfg: no more than max_records can wait, and every read synchronises the chain)
inline AnalyserReport analyser_report(fmr_chain *c, int stream, const fmr_analyser_config &cfg, const fmr_analyser_rule &rule) {
  AnalyserReport out;
  const int cap = cfg.max_records ? cfg.max_records : 64;
  const size_t row = 3 * (size_t)((cfg.fft_size ? cfg.fft_size : 4096) / 2 + 1);
  out.records.resize((size_t)cap);
  out.spectra.resize((size_t)cap * row);
  const int n = fmr_analyser_read(c, stream, out.records.data(), out.spectra.data(), cap, &out.info, sizeof out.info);
  if (n < 0) check(n, "fmr_analyser_read");
  out.records.resize((size_t)n);
  out.spectra.resize((size_t)n * row);
  if (n > 0)
    check(fmr_analyser_derive(out.records.data(), out.spectra.data(), n, &rule, sizeof rule, &out.levels, sizeof out.levels),
          "fmr_analyser_derive");
  return out;
}
inline fmr_analyser_rule analyser_rule(int view = 0, double tone_hz = 0.0) {
  fmr_analyser_rule r{};
  r.struct_size = sizeof r; r.view = view; r.tone_hz = tone_hz;
  return r;
}

// output stage (fmr_enable_output / fmr_output_read): everything that waits on one stream -- the PCM frames as bytes
// (interleaved int16 or float32, what AudioFileWriter::write_i16 / write_f32 take as they are) and the block records
struct OutputData {
  std::vector<unsigned char> pcm;
  size_t frames = 0;
  std::vector<fmr_output_block> blocks;
  fmr_output_info info{};
  const int16_t *s16() const { return reinterpret_cast<const int16_t *>(pcm.data()); }   // format FMR_PCM_S16
  const float *f32() const { return reinterpret_cast<const float *>(pcm.data()); }       // format FMR_PCM_F32
  size_t samples() const { return frames * (size_t)info.channels; }
};
inline fmr_output_config output_config(int format, double squelch_level, double gain, uint32_t max_frames, uint32_t max_blocks) {
  fmr_output_config m{};
  m.struct_size = sizeof m; m.format = format; m.squelch_level = squelch_level; m.gain = gain;
  m.max_frames = max_frames; m.max_blocks = max_blocks;
  return m;
}
inline fmr_output_rate_config output_rate_config(int rate, bool mono) {
  fmr_output_rate_config r{};
  r.struct_size = sizeof r; r.rate = rate; r.mono = mono ? 1 : 0;
  return r;
}
inline fmr_output_rate_info output_rate_info(fmr_chain *c, int stream) {
  fmr_output_rate_info info{};
  check(fmr_get_output_rate(c, stream, &info, sizeof info), "fmr_get_output_rate");
  return info;
}
inline OutputData output_data(fmr_chain *c, int stream) {
  OutputData out;
  int rc = fmr_output_read(c, stream, nullptr, 0, nullptr, 0, nullptr, &out.info, sizeof out.info);
  if (rc < 0) check(rc, "fmr_output_read");
  const size_t fb = (size_t)out.info.channels * (out.info.format == FMR_PCM_F32 ? 4 : 2);
  out.pcm.resize((size_t)out.info.frames_waiting * fb);
  out.blocks.resize((size_t)out.info.blocks_waiting);
  if (out.pcm.empty() && out.blocks.empty()) return out;
  rc = fmr_output_read(c, stream, out.pcm.data(), (size_t)out.info.frames_waiting, out.blocks.data(), (int)out.blocks.size(),
                       &out.frames, &out.info, sizeof out.info);
  if (rc < 0) check(rc, "fmr_output_read");
  out.pcm.resize(out.frames * fb);
  out.blocks.resize((size_t)rc);
  return out;
}

// MPX output (fmr_enable_mpx_output / fmr_mpx_output_read): everything that waits on one stream -- mono frames as bytes
// (int16 or float32 at info.rate, what AudioFileWriter::write_i16 / write_f32 take as they are)
struct MpxOutputData {
  std::vector<unsigned char> pcm;
  size_t frames = 0;
  fmr_mpx_output_info info{};
  const int16_t *s16() const { return reinterpret_cast<const int16_t *>(pcm.data()); }   // format FMR_PCM_S16
  const float *f32() const { return reinterpret_cast<const float *>(pcm.data()); }       // format FMR_PCM_F32
};
inline fmr_mpx_output_config mpx_output_config(int format, int rate, double gain, uint32_t max_frames) {
  fmr_mpx_output_config m{};
  m.struct_size = sizeof m; m.format = format; m.rate = rate; m.gain = gain; m.max_frames = max_frames;
  return m;
}
inline MpxOutputData mpx_output_data(fmr_chain *c, int stream) {
  MpxOutputData out;
  int rc = fmr_mpx_output_read(c, stream, nullptr, 0, nullptr, &out.info, sizeof out.info);
  if (rc < 0) check(rc, "fmr_mpx_output_read");
  const size_t fb = out.info.format == FMR_PCM_F32 ? 4 : 2;
  out.pcm.resize((size_t)out.info.frames_waiting * fb);
  if (out.pcm.empty()) return out;
  rc = fmr_mpx_output_read(c, stream, out.pcm.data(), (size_t)out.info.frames_waiting, &out.frames, &out.info, sizeof out.info);
  if (rc < 0) check(rc, "fmr_mpx_output_read");
  out.pcm.resize(out.frames * fb);
  return out;
}

// The optional stages a decoder object has enabled on its chain, each with its configuration.  The members enable a stage
// (fmr_enable_*: before the first process(), once) and remember it; apply() enables on a chain made anew -- for a front
// end, for RDS, for a larger batch -- what the one before it had.  A stage added here is added to apply().
struct Stages {
  std::optional<fmr_monitor_config> mon;
  std::optional<fmr_loudness_config> ld;
  std::optional<fmr_weak_signal_config> ws;
  std::optional<fmr_iq_correction_config> iqc;
  std::optional<fmr_blanker_config> nb;
  std::optional<fmr_rf_monitor_config> rf;
  std::optional<fmr_output_config> out;
  fmr_output_rate_config out_rate{};
  std::optional<fmr_analyser_config> an;
  std::optional<fmr_mpx_output_config> mpx;

  void monitor(fmr_chain *c, uint32_t interval_samples, int hist_bins, double hist_range, int max_records) {
    fmr_monitor_config m{};
    m.interval_samples = interval_samples; m.hist_bins = hist_bins; m.hist_range = hist_range; m.max_records = max_records;
    enable(c, mon, m, fmr_enable_monitor, "fmr_enable_monitor");
  }
  void loudness(fmr_chain *c, uint32_t step_samples, int max_records) {
    fmr_loudness_config m{};
    m.step_samples = step_samples; m.max_records = max_records;
    enable(c, ld, m, fmr_enable_loudness, "fmr_enable_loudness");
  }
  void weak_signal(fmr_chain *c, const fmr_weak_signal_config &m) { enable(c, ws, m, fmr_enable_weak_signal, "fmr_enable_weak_signal"); }
  void iq_correction(fmr_chain *c, const fmr_iq_correction_config &m) { enable(c, iqc, m, fmr_enable_iq_correction, "fmr_enable_iq_correction"); }
  void blanker(fmr_chain *c, const fmr_blanker_config &m) { enable(c, nb, m, fmr_enable_blanker, "fmr_enable_blanker"); }
  void rf_monitor(fmr_chain *c, uint32_t interval_samples, int max_records) {
    fmr_rf_monitor_config m{};
    m.interval_samples = interval_samples; m.max_records = max_records;
    enable(c, rf, m, fmr_enable_rf_monitor, "fmr_enable_rf_monitor");
  }
  // (fmr_set_output_rate behind it when a rate or mono is asked for)
  void output(fmr_chain *c, const fmr_output_config &m, const fmr_output_rate_config &r) {
    enable(c, out, m, fmr_enable_output, "fmr_enable_output");
    out_rate = r;
    if (r.rate != 0 || r.mono != 0) check(fmr_set_output_rate(c, &r, sizeof r), "fmr_set_output_rate");
  }
  void analyser(fmr_chain *c, int fft_size, uint32_t interval_samples, int max_records) {
    fmr_analyser_config m{};
    m.fft_size = fft_size; m.interval_samples = interval_samples; m.max_records = max_records;
    enable(c, an, m, fmr_enable_analyser, "fmr_enable_analyser");
  }
  fmr_analyser_config analyser_cfg() const { return an.value_or(fmr_analyser_config{}); }      // (what analyser_report sizes its read by)
  void mpx_output(fmr_chain *c, const fmr_mpx_output_config &m) { enable(c, mpx, m, fmr_enable_mpx_output, "fmr_enable_mpx_output"); }

  void apply(fmr_chain *c) {
    if (mon) enable(c, mon, *mon, fmr_enable_monitor, "fmr_enable_monitor");
    if (ld) enable(c, ld, *ld, fmr_enable_loudness, "fmr_enable_loudness");
    if (ws) weak_signal(c, *ws);
    if (iqc) iq_correction(c, *iqc);
    if (nb) blanker(c, *nb);
    if (rf) enable(c, rf, *rf, fmr_enable_rf_monitor, "fmr_enable_rf_monitor");
    if (out) output(c, *out, fmr_output_rate_config(out_rate));
    if (an) enable(c, an, *an, fmr_enable_analyser, "fmr_enable_analyser");
    if (mpx) mpx_output(c, *mpx);
  }

private:
  template <class Cfg, class Fn>
  static void enable(fmr_chain *c, std::optional<Cfg> &slot, Cfg m, Fn *fn, const char *name) {
    m.struct_size = sizeof m;
    check(fn(c, &m, sizeof m), name);
    slot = m;
  }
};
}  // namespace fmr_detail
using OutputData = fmr_detail::OutputData;
using MpxOutputData = fmr_detail::MpxOutputData;
using RfRecord = fmr_detail::RfRecord;
using ModulationRecord = fmr_detail::ModulationRecord;
using LoudnessReport = fmr_detail::LoudnessReport;
using WeakSignalReport = fmr_detail::WeakSignalReport;
using BlankerReport = fmr_detail::BlankerReport;
using IqCorrectionReport = fmr_detail::IqCorrectionReport;
using AnalyserReport = fmr_detail::AnalyserReport;

// FilterParameters (include/FilterParameters.h:31-49): tables served by the library.
struct FilterParameters {
  static IQSampleCoeff iq(const char *name) {
    const void *p = nullptr;
    int dbl = 0;
    const int n = fmr_filter_table(name, &p, &dbl);
    if (n < 0 || dbl) { fmr_detail::fail("unknown IQ filter table"); return {}; }
    const float *f = static_cast<const float *>(p);
    return IQSampleCoeff(f, f + n);
  }
  static SampleCoeff audio(const char *name) {
    const void *p = nullptr;
    int dbl = 0;
    const int n = fmr_filter_table(name, &p, &dbl);
    if (n < 0 || !dbl) { fmr_detail::fail("unknown audio filter table"); return {}; }
    const double *f = static_cast<const double *>(p);
    return SampleCoeff(f, f + n);
  }
  static inline const IQSampleCoeff delay_3taps_only_iq = {0.0f, 1.0f, 0.0f};
  static inline const IQSampleCoeff jj1bdx_fm_384kHz_narrow = iq("jj1bdx_fm_384kHz_narrow");
  static inline const IQSampleCoeff jj1bdx_fm_384kHz_medium = iq("jj1bdx_fm_384kHz_medium");
  static inline const IQSampleCoeff jj1bdx_am_48khz_narrow = iq("jj1bdx_am_48khz_narrow");
  static inline const IQSampleCoeff jj1bdx_am_48khz_medium = iq("jj1bdx_am_48khz_medium");
  static inline const IQSampleCoeff jj1bdx_am_48khz_default = iq("jj1bdx_am_48khz_default");
  static inline const IQSampleCoeff jj1bdx_am_48khz_wide = iq("jj1bdx_am_48khz_wide");
  static inline const IQSampleCoeff jj1bdx_nbfm_48khz_default = iq("jj1bdx_nbfm_48khz_default");
  static inline const IQSampleCoeff jj1bdx_nbfm_48khz_narrow = iq("jj1bdx_nbfm_48khz_narrow");
  static inline const IQSampleCoeff jj1bdx_nbfm_48khz_medium = iq("jj1bdx_nbfm_48khz_medium");
  static inline const IQSampleCoeff jj1bdx_nbfm_48khz_wide = iq("jj1bdx_nbfm_48khz_wide");
  static inline const SampleCoeff jj1bdx_48khz_fmaudio = audio("jj1bdx_48khz_fmaudio");
  static inline const SampleCoeff jj1bdx_48khz_nbfmaudio = audio("jj1bdx_48khz_nbfmaudio");
};

// FourthConverterIQ (FourthConverterIQ.h:30-82): Fs/4 shift, exact.  Stand-alone use costs a PCIe round trip per
// block; a decoder with attach_front_end(rate, true) applies the same shift inside its front-end kernel.
class FourthConverterIQ {
public:
  explicit FourthConverterIQ(bool up, int device = 0) : m_up(up) {
    fmr_config cfg{};
    cfg.device = device; cfg.n_streams = 1; cfg.mode = -1; cfg.input_rate = 384000.0;
    cfg.max_block_len = 65536; cfg.max_blocks = 1;
    m_chain = fmr_detail::make(cfg);
  }
  ~FourthConverterIQ() { fmr_destroy(m_chain); }
  FourthConverterIQ(const FourthConverterIQ &) = delete;
  FourthConverterIQ &operator=(const FourthConverterIQ &) = delete;
  void process(const IQSampleVector &samples_in, IQSampleVector &samples_out) {
    samples_out.resize(samples_in.size());
    fmr_detail::check(fmr_fourth_convert(m_chain, reinterpret_cast<const float *>(samples_in.data()), samples_in.size(),
                                         reinterpret_cast<float *>(samples_out.data()), m_up ? 1 : 0, &m_index),
                      "fmr_fourth_convert");
  }

private:
  fmr_chain *m_chain = nullptr;
  unsigned m_index = 0;          // FourthConverterIQ.h:31
  const bool m_up;
};

// IfResampler::process(const IQSampleVector&, IQSampleVector&)  (IfResampler.h:35-38), any pair of integer rates the
// resampler design covers (384 kHz for FM, 48 kHz for the AM / NBFM decoders, main.cpp:775-777).  Equal rates: a copy
// (main.cpp does not call process() then, :778,925-929).
class IfResampler {
public:
  static constexpr int max_input_length = 65536;   // IfResampler.h:31
  // resampler_class: FMR_RESAMPLER_R8B (default) -- the defaults of the r8b::CDSPResampler24 this class wraps in the
  // reference (IfResampler.cpp:25-29: 2 % transition band ending at Nyquist, 180 dB), so that the decoder behind it is
  // fed what the reference's filter delivers; FMR_RESAMPLER_FAST -- the throughput specification of the benchmark (a
  // narrower pass band at 140 dB: 5.5e-6 from R8B in the audio on a clean band, not for a crowded one)
  IfResampler(const double input_rate, const double output_rate, int device = 0, int resampler_class = FMR_RESAMPLER_R8B) {
    if (input_rate == output_rate) return;
    fmr_config cfg{};
    cfg.device = device; cfg.n_streams = 1; cfg.mode = -1; cfg.input_rate = input_rate; cfg.output_rate = output_rate;
    cfg.enable_resampler = 1; cfg.max_block_len = max_input_length; cfg.max_blocks = 1; cfg.resampler_class = resampler_class;
    m_chain = fmr_detail::make(cfg);
    m_rate = input_rate;
  }
  ~IfResampler() { if (m_chain) fmr_destroy(m_chain); }
  IfResampler(const IfResampler &) = delete;
  IfResampler &operator=(const IfResampler &) = delete;
  void process(const IQSampleVector &samples_in, IQSampleVector &samples_out) {
    if (!m_chain) { samples_out = samples_in; return; }
    samples_out.resize(samples_in.size() + 64);
    size_t n = 0;
    fmr_detail::check(fmr_resample(m_chain, reinterpret_cast<const float *>(samples_in.data()), samples_in.size(),
                                   reinterpret_cast<float *>(samples_out.data()), samples_out.size(), &n),
                      "fmr_resample");
    samples_out.resize(n);
  }
  // Impulse blanker on the input (no counterpart in the reference; fmr_enable_blanker): before the first process(), once;
  // cfg: the fields to set (zeros = the defaults; mode FMR_NB_MEASURE records only, FMR_NB_ACT zeroes the gated samples in
  // what the resampler reads).  read_blanker() drains the complete records and pools them.
  void enable_blanker(fmr_blanker_config cfg = fmr_blanker_config{}) {
    if (!m_chain) fmr_detail::fail("IfResampler::enable_blanker: equal rates, nothing is resampled");
    m_stages.blanker(m_chain, cfg);
  }
  BlankerReport read_blanker() { return fmr_detail::blanker_report(m_chain, 0, m_rate); }
  // DC-offset and IQ-imbalance correction of the same input (fmr_enable_iq_correction), under the same rules as
  // enable_blanker() and before or after it: cfg holds the fields to set (zeros = the defaults; FMR_IQC_MEASURE records
  // only, FMR_IQC_ACT corrects what the blanker and the front end read).  read_iq_correction() drains the complete
  // records and pools them.
  void enable_iq_correction(fmr_iq_correction_config cfg = fmr_iq_correction_config{}) {
    if (!m_chain) fmr_detail::fail("IfResampler::enable_iq_correction: equal rates, nothing is resampled");
    m_stages.iq_correction(m_chain, cfg);
  }
  IqCorrectionReport read_iq_correction() { return fmr_detail::iq_correction_report(m_chain, 0); }

private:
  fmr_chain *m_chain = nullptr;
  double m_rate = 0.0;
  fmr_detail::Stages m_stages;
};

// PilotPhaseLock::PpsEvent (PilotPhaseLock.h:40-44)
struct PilotPhaseLock {
  struct PpsEvent {
    std::uint64_t pps_index;
    std::uint64_t sample_index;
    double block_position;
  };
};

// FmDecoder (FmDecode.h:63-105)
class FmDecoder {
public:
  static constexpr double sample_rate_if = 384000;
  static constexpr double sample_rate_pcm = 48000;
  static constexpr double freq_dev = 75000;
  static constexpr double deemphasis_time_eu = 50;
  static constexpr double deemphasis_time_na = 75;

  FmDecoder(bool fmfilter_enable, IQSampleCoeff &fmfilter_coeff, bool stereo, double deemphasis, bool pilot_shift,
            unsigned int multipath_stages, int device = 0)
      : m_stereo(stereo) {
    m_cfg = fmr_config{};
    m_cfg.device = device; m_cfg.n_streams = 1; m_cfg.mode = FMR_MODE_FM; m_cfg.input_rate = sample_rate_if;
    m_cfg.fmfilter_enable = fmfilter_enable; m_cfg.filter_coeff = fmfilter_coeff.data();
    m_cfg.n_filter_coeff = (int)fmfilter_coeff.size(); m_cfg.stereo = stereo; m_cfg.deemphasis_us = deemphasis;
    m_cfg.pilot_shift = pilot_shift; m_cfg.multipath_stages = multipath_stages;
    m_cfg.max_block_len = 65536; m_cfg.max_blocks = 1;
    m_chain = fmr_detail::make(m_cfg);
  }
  ~FmDecoder() { fmr_destroy(m_chain); }
  FmDecoder(const FmDecoder &) = delete;
  FmDecoder &operator=(const FmDecoder &) = delete;

  // Fuse FourthConverterIQ + IfResampler into this decoder's chain: process() then takes
  // the source-rate IQ block (what main.cpp:889 pulls) and the IF never leaves the GPU.
  void attach_front_end(double input_rate, bool fourth_down, int resampler_class = FMR_RESAMPLER_R8B) {
    fmr_destroy(m_chain);
    m_cfg.input_rate = input_rate; m_cfg.enable_resampler = 1; m_cfg.enable_fourth_down = fourth_down;
    m_cfg.resampler_class = resampler_class;
    m_chain = fmr_detail::make(m_cfg, m_rds);
    m_stages.apply(m_chain);
  }

  // RDS (no counterpart in the reference; fmr_create_rds): re-creates the chain with the RDS decoder, before the first
  // process().  get_rds_groups() drains the groups decoded so far; rds_station() holds PI / PTY / PS / RadioText.
  void enable_rds() {
    if (m_started) fmr_detail::fail("FmDecoder::enable_rds: after the first process()");
    m_rds = true;
    fmr_destroy(m_chain);
    m_chain = fmr_detail::make(m_cfg, true);
    m_stages.apply(m_chain);
  }
  // error correction of the RDS blocks (fmr_set_rds_correction: FMR_RDS_FEC_OFF / _BURST / _SOFT; 0 = the defaults); at
  // any time after enable_rds(), from the decoder's next block boundary on.  enable_rds() starts with it off.
  void set_rds_correction(int mode, int max_burst = 0, int soft_symbols = 0, double soft_max_cost = 0.0) {
    fmr_detail::rds_correction(m_chain, mode, max_burst, soft_symbols, soft_max_cost);
  }
  std::vector<fmr_rds_group> get_rds_groups() { return fmr_detail::rds_groups(m_chain, 0, m_station); }
  const fmr_rds::Station &rds_station() { get_rds_groups(); return m_station; }

  // Modulation monitor (no counterpart in the reference; fmr_enable_monitor): records of interval_samples MPX samples
  // (0 = one second) with peak deviation, MPX power, pilot and RDS injection; before the first process(), once.
  // read_modulation_records() drains the complete ones, oldest first.
  void enable_modulation_monitor(uint32_t interval_samples = 0, int hist_bins = 0, double hist_range = 0.0, int max_records = 0) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_modulation_monitor: after the first process()");
    m_stages.monitor(m_chain, interval_samples, hist_bins, hist_range, max_records);
  }
  std::vector<ModulationRecord> read_modulation_records() { return fmr_detail::monitor_records(m_chain, 0); }

  // Audio monitor (the level meter main.cpp prints beside the IF level, on the device; fmr_enable_loudness): records of
  // step_samples audio samples (0 = 4800) with K-weighted power, sample and true peak, L/R sums; before the first
  // process(), once.  read_loudness() drains the complete ones and derives loudness, peaks, correlation and silence.
  void enable_loudness(uint32_t step_samples = 0, int max_records = 0) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_loudness: after the first process()");
    m_stages.loudness(m_chain, step_samples, max_records);
  }
  LoudnessReport read_loudness(double silence_dbfs = -60.0) { return fmr_detail::loudness_report(m_chain, 0, silence_dbfs); }

  // Weak-signal handling (no counterpart in the reference; fmr_enable_weak_signal): stereo blend, high cut and soft mute
  // driven by the MPX's ultrasonic noise; before the first process(), once.  cfg: the fields to set (zeros = the defaults;
  // mode FMR_WS_MEASURE records only, FMR_WS_ACT also rewrites the audio process() returns).  read_weak_signal() drains
  // the complete records and pools them.
  void enable_weak_signal(fmr_weak_signal_config cfg = fmr_weak_signal_config{}) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_weak_signal: after the first process()");
    m_stages.weak_signal(m_chain, cfg);
  }
  WeakSignalReport read_weak_signal() { return fmr_detail::weak_signal_report(m_chain, 0); }

  // Impulse blanker on the source-rate input (no counterpart in the reference; fmr_enable_blanker): after
  // attach_front_end() (the stage sits in front of the IF resampler), before the first process(), once.  cfg: the fields
  // to set (zeros = the defaults; FMR_NB_MEASURE records only, FMR_NB_ACT zeroes the gated samples in what the front end
  // reads).  read_blanker() drains the complete records and pools them.
  void enable_blanker(fmr_blanker_config cfg = fmr_blanker_config{}) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_blanker: after the first process()");
    m_stages.blanker(m_chain, cfg);
  }
  BlankerReport read_blanker() { return fmr_detail::blanker_report(m_chain, 0, m_cfg.input_rate); }
  // DC-offset and IQ-imbalance correction of the same input (fmr_enable_iq_correction), under the same rules as
  // enable_blanker() and before or after it: cfg holds the fields to set (zeros = the defaults; FMR_IQC_MEASURE records
  // only, FMR_IQC_ACT corrects what the blanker and the front end read).  read_iq_correction() drains the complete
  // records and pools them.
  void enable_iq_correction(fmr_iq_correction_config cfg = fmr_iq_correction_config{}) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_iq_correction: after the first process()");
    m_stages.iq_correction(m_chain, cfg);
  }
  IqCorrectionReport read_iq_correction() { return fmr_detail::iq_correction_report(m_chain, 0); }

  // RF monitor (no counterpart in the reference; fmr_enable_rf_monitor): records of interval_samples IF samples (0 =
  // 38400, 100 ms) with level, C/N, envelope AM and fade percentiles; before the first process(), once.
  // read_rf_records() drains the complete ones, oldest first.
  void enable_rf_monitor(uint32_t interval_samples = 0, int max_records = 0) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_rf_monitor: after the first process()");
    m_stages.rf_monitor(m_chain, interval_samples, max_records);
  }
  std::vector<RfRecord> read_rf_records() { return fmr_detail::rf_records(m_chain, 0); }

  // Output stage (what main.cpp:976-1002 does behind the decoder, on the device; fmr_enable_output): the squelched and
  // scaled audio as FMR_PCM_S16 / FMR_PCM_F32 frames and one record per block with the IF / AF meters; before the first
  // process(), once.  squelch_level is linear (fmr_squelch_level_from_db gives it from -l dB; 0 = never closed), gain 0 =
  // 0.5.  rate / mono: the PCM ring at that rate (8000 .. 48000, fmr_set_output_rate) and / or downmixed to one channel.
  // read_output() drains everything that waits.
  void enable_output(int format = FMR_PCM_S16, double squelch_level = 0.0, double gain = 0.0, uint32_t max_frames = 0,
                     uint32_t max_blocks = 0, int rate = 0, bool mono = false) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_output: after the first process()");
    m_stages.output(m_chain, fmr_detail::output_config(format, squelch_level, gain, max_frames, max_blocks),
                    fmr_detail::output_rate_config(rate, mono));
  }
  OutputData read_output() { return fmr_detail::output_data(m_chain, 0); }
  fmr_output_rate_info output_rate_info() { return fmr_detail::output_rate_info(m_chain, 0); }
  // MPX output (no counterpart in the reference; fmr_enable_mpx_output): the composite baseband as mono FMR_PCM_S16 /
  // FMR_PCM_F32 frames at `rate` (0 = 384000, the MPX as it is; 96000 .. 384000, e.g. 192000, 171000, 228000); gain 0 = 0.5
  // (full scale +-150 kHz); before the first process(), once.  read_mpx_output() drains everything that waits.
  void enable_mpx_output(int format = FMR_PCM_S16, int rate = 192000, double gain = 0.0, uint32_t max_frames = 0) {
    if (m_started) fmr_detail::fail("FmDecoder::enable_mpx_output: after the first process()");
    m_stages.mpx_output(m_chain, fmr_detail::mpx_output_config(format, rate, gain, max_frames));
  }
  MpxOutputData read_mpx_output() { return fmr_detail::mpx_output_data(m_chain, 0); }
  // Audio analyser (the spectrum analyser the reference's author judges receivers with, on the device;
  // fmr_enable_analyser): records of interval_samples audio frames (0 = 6 fft_size) with the Blackman-Harris power spectra
  // of the channels; before the first process(), once.  read_analyser() drains the complete ones and derives tone, THD,
  // THD+N, SINAD and noise of all of them pooled (view 0 = L .. 3 = S; tone_hz 0 = the strongest bin of 20 Hz .. 15 kHz).
  void enable_analyser(int fft_size = 0, uint32_t interval_samples = 0, int max_records = 0) {
    m_stages.analyser(m_chain, fft_size, interval_samples, max_records);
  }
  AnalyserReport read_analyser(int view = 0, double tone_hz = 0.0) {
    return fmr_detail::analyser_report(m_chain, 0, m_stages.analyser_cfg(), fmr_detail::analyser_rule(view, tone_hz));
  }

  // Latency for throughput: hold back `blocks` - 1 calls and decode `blocks` blocks in ONE batched call.  process()
  // then returns an empty vector ("nothing yet": the contract of FmDecode.cpp:89-92,185-188, which main.cpp:981-984
  // already handles) until the batch is full, and the audio of all its blocks at once.  One 65536-sample block per
  // call costs ~0.3 ms, almost all of it launch overhead (~85 kernel launches); a batch costs about the same.
  // Default 1 = the reference's call-by-call behaviour.
  //  * END OF STREAM: call flush() -- it decodes the blocks still held back (fewer than a batch).  Without it up to
  //    blocks - 1 source blocks of audio would be lost; the reference decodes every block.
  //  * The status getters (get_if_rms(), get_pps_events(), ...) describe the LAST block of the batch just decoded, the
  //    PPS events all of its blocks.
  //  * Raising the batch above the chain's capacity re-creates the chain and is therefore only possible before the first
  //    process(); lowering it (or raising it again up to the capacity) is possible at any time and keeps held-back blocks.
  void set_batch_blocks(unsigned blocks) {
    if (blocks < 1) blocks = 1;
    if (blocks == m_batch) return;
    if (blocks > m_capacity) {
      if (m_started) fmr_detail::fail("FmDecoder::set_batch_blocks: a larger batch than the chain was created for, after the first process()");
      fmr_destroy(m_chain);
      m_cfg.max_blocks = (int)blocks;
      m_chain = fmr_detail::make(m_cfg, m_rds);
      m_stages.apply(m_chain);
      m_capacity = blocks;
    }
    m_batch = blocks;
  }

  // samples_in by value, audio resized by the callee, empty = "nothing yet" (FmDecode.cpp:85-92)
  void process(IQSampleVector samples_in, SampleVector &audio) {
    m_pps_fetched = false;       // PilotPhaseLock::process clears m_pps_events on every call (PilotPhaseLock.cpp:62)
    m_pps.clear();
    m_started = true;
    if (m_batch > 1 || !m_pending_len.empty()) {
      m_pending.insert(m_pending.end(), samples_in.begin(), samples_in.end());
      m_pending_len.push_back((uint32_t)samples_in.size());
      audio.clear();
      if (m_pending_len.size() < m_batch) { m_pps_fetched = true; return; }
      decode_pending(audio);
      return;
    }
    audio.resize(2 * (samples_in.size() + 64));
    size_t n = 0;
    fmr_detail::check(fmr_process(m_chain, reinterpret_cast<const float *>(samples_in.data()), samples_in.size(),
                                  audio.data(), audio.size(), &n),
                      "fmr_process");
    audio.resize(n);
  }
  // Decode whatever set_batch_blocks() is still holding back (end of stream, or before a batch-size change that must
  // not add latency).  audio is empty if nothing was pending.
  void flush(SampleVector &audio) {
    m_pps_fetched = false;
    m_pps.clear();
    audio.clear();
    if (m_pending_len.empty()) { m_pps_fetched = true; return; }
    decode_pending(audio);
  }
  size_t pending_blocks() const { return m_pending_len.size(); }
  bool stereo_detected() { return status().stereo_detected != 0; }
  float get_tuning_offset() { return status().baseband_mean * freq_dev; }
  float get_baseband_level() { return status().baseband_level; }
  double get_pilot_level() { return status().pilot_level; }
  float get_if_rms() { return status().if_rms; }
  double get_multipath_error() { return status().multipath_error; }
  // Events of the most recent process() call; erase_first_pps_event() consumes them one by one (main.cpp:1087-1094).
  std::vector<PilotPhaseLock::PpsEvent> get_pps_events() {
    fetch_pps();
    return m_pps;
  }
  void erase_first_pps_event() {
    fetch_pps();
    if (!m_pps.empty()) m_pps.erase(m_pps.begin());
  }
  const std::vector<std::complex<float>> &get_multipath_coefficients() {
    m_coeff.resize(1300);
    const int n = fmr_get_multipath_coefficients(m_chain, 0, reinterpret_cast<float *>(m_coeff.data()), 2600);
    m_coeff.resize(n > 0 ? n : 0);
    return m_coeff;
  }

private:
  fmr_status status() {
    fmr_status st{};
    fmr_detail::check(fmr_get_status(m_chain, 0, &st), "fmr_get_status");
    return st;
  }
  // the held-back blocks in calls of at most the chain's capacity (fmr_process_blocks takes any count up to max_blocks)
  void decode_pending(SampleVector &audio) {
    audio.resize(2 * (m_pending.size() + 64 * m_pending_len.size()));
    size_t done_blocks = 0, done_samples = 0, n_audio = 0;
    while (done_blocks < m_pending_len.size()) {
      const size_t nb = std::min<size_t>(m_capacity, m_pending_len.size() - done_blocks);
      size_t ns = 0;
      for (size_t b = 0; b < nb; b++) ns += m_pending_len[done_blocks + b];
      std::vector<uint32_t> alen(nb);
      fmr_detail::check(fmr_process_blocks(m_chain, reinterpret_cast<const float *>(m_pending.data() + done_samples), ns,
                                           m_pending_len.data() + done_blocks, (int)nb, audio.data() + n_audio,
                                           audio.size() - n_audio, alen.data()),
                        "fmr_process_blocks");
      for (uint32_t v : alen) n_audio += v;
      done_blocks += nb; done_samples += ns;
    }
    audio.resize(n_audio);
    m_pending.clear();
    m_pending_len.clear();
  }
  void fetch_pps() {
    if (m_pps_fetched) return;
    fmr_pps_event ev[64];
    const int n = fmr_get_pps_events(m_chain, 0, ev, 64);
    m_pps.clear();
    for (int i = 0; i < n && i < 64; i++) m_pps.push_back({ev[i].pps_index, ev[i].sample_index, ev[i].block_position});
    m_pps_fetched = true;
  }
  fmr_config m_cfg{};
  fmr_detail::Stages m_stages;
  fmr_chain *m_chain = nullptr;
  bool m_rds = false;
  fmr_rds::Station m_station;
  bool m_stereo;
  bool m_pps_fetched = true;
  std::vector<PilotPhaseLock::PpsEvent> m_pps;
  unsigned m_batch = 1, m_capacity = 1;
  bool m_started = false;
  IQSampleVector m_pending;
  std::vector<uint32_t> m_pending_len;
  std::vector<std::complex<float>> m_coeff;
};

// MpxDecoder (no counterpart in the reference; fmr_create_mpx_decoder): FmDecoder's decoder behind a composite input -- an
// MPX archive (MpxFileReader, fmradion_fileio.hpp), a stereo generator's output from a 192 kHz sound card -- as mono
// FMR_PCM_S16 / FMR_PCM_F32 frames at `rate` (0 = 384000).  gain 0 = 2.0, the inverse of the MPX output's default.  It has
// the getters of FmDecoder that still have a meaning: there is no IF level, no equaliser.
class MpxDecoder {
public:
  MpxDecoder(int rate, int format, bool stereo, double deemphasis = FmDecoder::deemphasis_time_eu, bool pilot_shift = false,
             double gain = 0.0, bool rds = false, int device = 0)
      : m_format(format) {
    fmr_config cfg{};
    cfg.struct_size = sizeof cfg;
    cfg.device = device; cfg.n_streams = 1; cfg.mode = FMR_MODE_FM; cfg.stereo = stereo; cfg.deemphasis_us = deemphasis;
    cfg.pilot_shift = pilot_shift; cfg.max_block_len = 65536; cfg.max_blocks = 1;
    fmr_mpx_input_config in{};
    in.struct_size = sizeof in; in.format = format; in.rate = rate; in.gain = gain; in.rds = rds ? 1 : 0;
    fmr_detail::check(fmr_create_mpx_decoder(&cfg, sizeof cfg, &in, sizeof in, &m_chain), "fmr_create_mpx_decoder");
  }
  ~MpxDecoder() { fmr_destroy(m_chain); }
  MpxDecoder(const MpxDecoder &) = delete;
  MpxDecoder &operator=(const MpxDecoder &) = delete;

  // one block of frames (at most 65536) in, interleaved audio out; the vector's type must be the decoder's format
  void process(const std::vector<float> &frames, SampleVector &audio) {
    if (m_format != FMR_PCM_F32) fmr_detail::fail("MpxDecoder::process(float): the decoder was made for FMR_PCM_S16");
    run(frames.data(), frames.size(), audio);
  }
  void process(const std::vector<int16_t> &frames, SampleVector &audio) {
    if (m_format != FMR_PCM_S16) fmr_detail::fail("MpxDecoder::process(int16_t): the decoder was made for FMR_PCM_F32");
    run(frames.data(), frames.size(), audio);
  }
  fmr_mpx_input_info input_info() {
    fmr_mpx_input_info i{};
    fmr_detail::check(fmr_get_mpx_input_info(m_chain, 0, &i, sizeof i), "fmr_get_mpx_input_info");
    return i;
  }
  bool stereo_detected() { return status().stereo_detected != 0; }
  float get_tuning_offset() { return status().baseband_mean * (float)FmDecoder::freq_dev; }
  float get_baseband_level() { return status().baseband_level; }
  double get_pilot_level() { return status().pilot_level; }
  // events of the most recent process() call
  std::vector<PilotPhaseLock::PpsEvent> get_pps_events() {
    fmr_pps_event ev[64];
    const int n = fmr_get_pps_events(m_chain, 0, ev, 64);
    std::vector<PilotPhaseLock::PpsEvent> out;
    for (int i = 0; i < n && i < 64; i++) out.push_back({ev[i].pps_index, ev[i].sample_index, ev[i].block_position});
    return out;
  }
  // with rds = true: as FmDecoder's
  void set_rds_correction(int mode, int max_burst = 0, int soft_symbols = 0, double soft_max_cost = 0.0) {
    fmr_detail::rds_correction(m_chain, mode, max_burst, soft_symbols, soft_max_cost);
  }
  std::vector<fmr_rds_group> get_rds_groups() { return fmr_detail::rds_groups(m_chain, 0, m_station); }
  const fmr_rds::Station &rds_station() { get_rds_groups(); return m_station; }
  // the stages an MPX decoder accepts, as FmDecoder's (before the first process(), once each)
  void enable_modulation_monitor(uint32_t interval_samples = 0, int hist_bins = 0, double hist_range = 0.0, int max_records = 0) {
    m_stages.monitor(m_chain, interval_samples, hist_bins, hist_range, max_records);
  }
  std::vector<ModulationRecord> read_modulation_records() { return fmr_detail::monitor_records(m_chain, 0); }
  void enable_loudness(uint32_t step_samples = 0, int max_records = 0) {
    m_stages.loudness(m_chain, step_samples, max_records);
  }
  LoudnessReport read_loudness(double silence_dbfs = -60.0) { return fmr_detail::loudness_report(m_chain, 0, silence_dbfs); }
  void enable_output(int format = FMR_PCM_S16, double gain = 0.0, uint32_t max_frames = 0, uint32_t max_blocks = 0, int rate = 0,
                     bool mono = false) {      // (no squelch: there is no IF level)
    m_stages.output(m_chain, fmr_detail::output_config(format, 0.0, gain, max_frames, max_blocks), fmr_detail::output_rate_config(rate, mono));
  }
  OutputData read_output() { return fmr_detail::output_data(m_chain, 0); }
  void enable_mpx_output(int format = FMR_PCM_S16, int rate = 192000, double gain = 0.0, uint32_t max_frames = 0) {
    m_stages.mpx_output(m_chain, fmr_detail::mpx_output_config(format, rate, gain, max_frames));
  }
  MpxOutputData read_mpx_output() { return fmr_detail::mpx_output_data(m_chain, 0); }

private:
  fmr_status status() {
    fmr_status st{};
    fmr_detail::check(fmr_get_status(m_chain, 0, &st), "fmr_get_status");
    return st;
  }
  void run(const void *frames, size_t n, SampleVector &audio) {
    audio.clear();
    if (n == 0) return;
    audio.resize(n + 128);      // (at most 4 MPX samples per frame, 2 doubles per 8 of them)
    uint32_t bl = (uint32_t)n, al = 0;
    fmr_detail::check(fmr_process_mpx_blocks(m_chain, frames, n, &bl, 1, audio.data(), audio.size(), &al), "fmr_process_mpx_blocks");
    audio.resize(al);
  }
  fmr_chain *m_chain = nullptr;
  int m_format;
  fmr_rds::Station m_station;
  fmr_detail::Stages m_stages;
};

// AmDecoder (AmDecode.h:48-65), all of its modes: AM, DSB, USB, LSB, CW, WSPR
class AmDecoder {
public:
  static constexpr double sample_rate_pcm = 48000;
  static constexpr double internal_rate_pcm = 48000;
  AmDecoder(IQSampleCoeff &amfilter_coeff, const ModType mode, int device = 0) {
    // main.cpp:813 constructs the AmDecoder whatever the mode; with an FM mode it is never used (AmDecode.cpp:96-147
    // has no case for it): build it as an AM decoder
    m_cfg = fmr_config{};
    m_cfg.device = device; m_cfg.n_streams = 1;
    m_cfg.mode = (mode == ModType::FM || mode == ModType::NBFM) ? FMR_MODE_AM : static_cast<int>(mode);   // FMR_MODE_* follow ModType
    m_cfg.input_rate = internal_rate_pcm; m_cfg.filter_coeff = amfilter_coeff.data();
    m_cfg.n_filter_coeff = (int)amfilter_coeff.size(); m_cfg.max_block_len = 65536; m_cfg.max_blocks = 1;
    m_chain = fmr_detail::make(m_cfg);
  }
  ~AmDecoder() { fmr_destroy(m_chain); }
  AmDecoder(const AmDecoder &) = delete;
  AmDecoder &operator=(const AmDecoder &) = delete;
  void attach_front_end(double input_rate, bool fourth_down, int resampler_class = FMR_RESAMPLER_R8B) {
    fmr_destroy(m_chain);
    m_cfg.input_rate = input_rate; m_cfg.enable_resampler = 1; m_cfg.enable_fourth_down = fourth_down;
    m_cfg.resampler_class = resampler_class;
    m_chain = fmr_detail::make(m_cfg);
    m_stages.apply(m_chain);
  }
  // Impulse blanker on the source-rate input (fmr_enable_blanker): after attach_front_end(), before the first process(),
  // once; cfg: the fields to set (zeros = the defaults).  read_blanker() drains the complete records and pools them.
  void enable_blanker(fmr_blanker_config cfg = fmr_blanker_config{}) {
    m_stages.blanker(m_chain, cfg);
  }
  BlankerReport read_blanker() { return fmr_detail::blanker_report(m_chain, 0, m_cfg.input_rate); }
  // DC-offset and IQ-imbalance correction of the same input (fmr_enable_iq_correction), under the same rules as
  // enable_blanker() and before or after it: cfg holds the fields to set (zeros = the defaults; FMR_IQC_MEASURE records
  // only, FMR_IQC_ACT corrects what the blanker and the front end read).  read_iq_correction() drains the complete
  // records and pools them.
  void enable_iq_correction(fmr_iq_correction_config cfg = fmr_iq_correction_config{}) {
    m_stages.iq_correction(m_chain, cfg);
  }
  IqCorrectionReport read_iq_correction() { return fmr_detail::iq_correction_report(m_chain, 0); }
  // Output stage (fmr_enable_output): squelch, gain, PCM frames and the per-block IF / AF meters on the device; before
  // the first process(), once.  rate: the PCM ring at that rate (fmr_set_output_rate).  read_output() drains everything
  // that waits.
  void enable_output(int format = FMR_PCM_S16, double squelch_level = 0.0, double gain = 0.0, uint32_t max_frames = 0,
                     uint32_t max_blocks = 0, int rate = 0, bool mono = false) {
    m_stages.output(m_chain, fmr_detail::output_config(format, squelch_level, gain, max_frames, max_blocks),
                    fmr_detail::output_rate_config(rate, mono));
  }
  OutputData read_output() { return fmr_detail::output_data(m_chain, 0); }
  fmr_output_rate_info output_rate_info() { return fmr_detail::output_rate_info(m_chain, 0); }
  // Audio analyser (the spectrum analyser the reference's author judges receivers with, on the device;
  // fmr_enable_analyser): records of interval_samples audio frames (0 = 6 fft_size) with the Blackman-Harris power spectra
  // of the channels; before the first process(), once.  read_analyser() drains the complete ones and derives tone, THD,
  // THD+N, SINAD and noise of all of them pooled (view 0 = L .. 3 = S; tone_hz 0 = the strongest bin of 20 Hz .. 15 kHz).
  void enable_analyser(int fft_size = 0, uint32_t interval_samples = 0, int max_records = 0) {
    m_stages.analyser(m_chain, fft_size, interval_samples, max_records);
  }
  AnalyserReport read_analyser(int view = 0, double tone_hz = 0.0) {
    return fmr_detail::analyser_report(m_chain, 0, m_stages.analyser_cfg(), fmr_detail::analyser_rule(view, tone_hz));
  }
  void process(IQSampleVector samples_in, SampleVector &audio) {
    audio.resize(samples_in.size() + 64);
    size_t n = 0;
    fmr_detail::check(fmr_process(m_chain, reinterpret_cast<const float *>(samples_in.data()), samples_in.size(),
                                  audio.data(), audio.size(), &n),
                      "fmr_process");
    audio.resize(n);
  }
  double get_baseband_level() { return status().baseband_level; }
  float get_af_agc_current_gain() { return (float)status().af_agc_gain; }
  float get_if_agc_current_gain() { return status().if_agc_gain; }
  float get_if_rms() { return status().if_rms; }

private:
  fmr_status status() {
    fmr_status st{};
    fmr_detail::check(fmr_get_status(m_chain, 0, &st), "fmr_get_status");
    return st;
  }
  fmr_config m_cfg{};
  fmr_detail::Stages m_stages;
  fmr_chain *m_chain = nullptr;
};

// NbfmDecoder (NbfmDecode.h:49-66)
class NbfmDecoder {
public:
  static constexpr double sample_rate_pcm = 48000;
  static constexpr double internal_rate_pcm = 48000;
  static constexpr double freq_dev_normal = 8000;
  static constexpr double freq_dev_wide = 17000;
  NbfmDecoder(IQSampleCoeff &nbfmfilter_coeff, const double freq_dev, int device = 0) : m_freq_dev(freq_dev) {
    m_cfg = fmr_config{};
    m_cfg.device = device; m_cfg.n_streams = 1; m_cfg.mode = FMR_MODE_NBFM; m_cfg.input_rate = internal_rate_pcm;
    m_cfg.filter_coeff = nbfmfilter_coeff.data(); m_cfg.n_filter_coeff = (int)nbfmfilter_coeff.size();
    m_cfg.nbfm_freq_dev = freq_dev; m_cfg.max_block_len = 65536; m_cfg.max_blocks = 1;
    m_chain = fmr_detail::make(m_cfg);
  }
  ~NbfmDecoder() { fmr_destroy(m_chain); }
  NbfmDecoder(const NbfmDecoder &) = delete;
  NbfmDecoder &operator=(const NbfmDecoder &) = delete;
  void attach_front_end(double input_rate, bool fourth_down, int resampler_class = FMR_RESAMPLER_R8B) {
    fmr_destroy(m_chain);
    m_cfg.input_rate = input_rate; m_cfg.enable_resampler = 1; m_cfg.enable_fourth_down = fourth_down;
    m_cfg.resampler_class = resampler_class;
    m_chain = fmr_detail::make(m_cfg);
    m_stages.apply(m_chain);
  }
  // Impulse blanker on the source-rate input (fmr_enable_blanker): after attach_front_end(), before the first process(),
  // once; cfg: the fields to set (zeros = the defaults).  read_blanker() drains the complete records and pools them.
  void enable_blanker(fmr_blanker_config cfg = fmr_blanker_config{}) {
    m_stages.blanker(m_chain, cfg);
  }
  BlankerReport read_blanker() { return fmr_detail::blanker_report(m_chain, 0, m_cfg.input_rate); }
  // DC-offset and IQ-imbalance correction of the same input (fmr_enable_iq_correction), under the same rules as
  // enable_blanker() and before or after it: cfg holds the fields to set (zeros = the defaults; FMR_IQC_MEASURE records
  // only, FMR_IQC_ACT corrects what the blanker and the front end read).  read_iq_correction() drains the complete
  // records and pools them.
  void enable_iq_correction(fmr_iq_correction_config cfg = fmr_iq_correction_config{}) {
    m_stages.iq_correction(m_chain, cfg);
  }
  IqCorrectionReport read_iq_correction() { return fmr_detail::iq_correction_report(m_chain, 0); }
  // Output stage (fmr_enable_output): squelch, gain, PCM frames and the per-block IF / AF meters on the device; before
  // the first process(), once.  rate: the PCM ring at that rate (fmr_set_output_rate).  read_output() drains everything
  // that waits.
  void enable_output(int format = FMR_PCM_S16, double squelch_level = 0.0, double gain = 0.0, uint32_t max_frames = 0,
                     uint32_t max_blocks = 0, int rate = 0, bool mono = false) {
    m_stages.output(m_chain, fmr_detail::output_config(format, squelch_level, gain, max_frames, max_blocks),
                    fmr_detail::output_rate_config(rate, mono));
  }
  OutputData read_output() { return fmr_detail::output_data(m_chain, 0); }
  fmr_output_rate_info output_rate_info() { return fmr_detail::output_rate_info(m_chain, 0); }
  // Audio analyser (the spectrum analyser the reference's author judges receivers with, on the device;
  // fmr_enable_analyser): records of interval_samples audio frames (0 = 6 fft_size) with the Blackman-Harris power spectra
  // of the channels; before the first process(), once.  read_analyser() drains the complete ones and derives tone, THD,
  // THD+N, SINAD and noise of all of them pooled (view 0 = L .. 3 = S; tone_hz 0 = the strongest bin of 20 Hz .. 15 kHz).
  void enable_analyser(int fft_size = 0, uint32_t interval_samples = 0, int max_records = 0) {
    m_stages.analyser(m_chain, fft_size, interval_samples, max_records);
  }
  AnalyserReport read_analyser(int view = 0, double tone_hz = 0.0) {
    return fmr_detail::analyser_report(m_chain, 0, m_stages.analyser_cfg(), fmr_detail::analyser_rule(view, tone_hz));
  }
  void process(const IQSampleVector &samples_in, SampleVector &audio) {
    audio.resize(samples_in.size() + 64);
    size_t n = 0;
    fmr_detail::check(fmr_process(m_chain, reinterpret_cast<const float *>(samples_in.data()), samples_in.size(),
                                  audio.data(), audio.size(), &n),
                      "fmr_process");
    audio.resize(n);
  }
  float get_tuning_offset() { return (float)(status().baseband_mean * m_freq_dev); }
  float get_baseband_level() { return status().baseband_level; }
  float get_if_rms() { return status().if_rms; }

private:
  fmr_status status() {
    fmr_status st{};
    fmr_detail::check(fmr_get_status(m_chain, 0, &st), "fmr_get_status");
    return st;
  }
  const double m_freq_dev;
  fmr_config m_cfg{};
  fmr_detail::Stages m_stages;
  fmr_chain *m_chain = nullptr;
};


// ChannelBank (no counterpart in the reference): K stations out of one wideband capture.  Channel k decodes the station
// at +offsets_hz[k] Hz in the capture's spectrum (fmr_config.channel_offset_hz) with the FmDecoder / AmDecoder /
// NbfmDecoder of `mode` behind an IfResampler of `resampler_class`; every channel shares that one configuration.
// filter_coeff is what the decoder of `mode` takes: FmDecoder's IF filter (used when fmfilter_enable), AmDecoder's
// amfilter_coeff (AM / DSB; USB / LSB / CW / WSPR use AmDecoder's built-in filters), NbfmDecoder's nbfmfilter_coeff.
// stereo / deemphasis / pilot_shift / multipath_stages are FmDecoder's and ignored by the other modes; nbfm_freq_dev is
// NbfmDecoder's freq_dev (0 = its default, 8000 Hz).
// process() takes the capture block once and returns one audio vector per channel; the getters take the channel.
class ChannelBank {
public:
  ChannelBank(double input_rate, const std::vector<int32_t> &offsets_hz, ModType mode, bool fmfilter_enable,
              IQSampleCoeff &filter_coeff, bool stereo, double deemphasis, bool pilot_shift, unsigned int multipath_stages,
              int resampler_class = FMR_RESAMPLER_R8B, int device = 0, size_t max_block_len = 65536,
              double nbfm_freq_dev = 0.0)
      : m_offsets(offsets_hz), m_max_block(max_block_len),
        m_freq_dev(mode == ModType::FM ? FmDecoder::freq_dev : nbfm_freq_dev > 0 ? nbfm_freq_dev : 8000.0) {
    if (m_offsets.empty()) fmr_detail::fail("ChannelBank: no channel");
    fmr_config cfg{};
    cfg.device = device; cfg.n_streams = (int)m_offsets.size(); cfg.mode = static_cast<int>(mode);
    cfg.input_rate = input_rate; cfg.enable_resampler = 1; cfg.resampler_class = resampler_class;
    cfg.fmfilter_enable = fmfilter_enable; cfg.filter_coeff = filter_coeff.data(); cfg.n_filter_coeff = (int)filter_coeff.size();
    cfg.stereo = stereo; cfg.deemphasis_us = deemphasis; cfg.pilot_shift = pilot_shift; cfg.multipath_stages = multipath_stages;
    cfg.max_block_len = max_block_len; cfg.max_blocks = 1; cfg.nbfm_freq_dev = nbfm_freq_dev;
    cfg.channel_offset_hz = m_offsets.data();
    m_cfg = cfg;
    m_chain = fmr_detail::make(cfg);
  }
  ~ChannelBank() { fmr_destroy(m_chain); }
  ChannelBank(const ChannelBank &) = delete;
  ChannelBank &operator=(const ChannelBank &) = delete;

  size_t channels() const { return m_offsets.size(); }
  int32_t offset_hz(size_t ch) const { return m_offsets.at(ch); }

  // RDS of every channel (fmr_create_rds): re-creates the chain with the RDS decoder, before the first process()
  void enable_rds() {
    fmr_destroy(m_chain);
    m_cfg.channel_offset_hz = m_offsets.data();
    m_chain = fmr_detail::make(m_cfg, true);
    m_stages.apply(m_chain);
    m_stations.assign(m_offsets.size(), fmr_rds::Station());
  }
  // error correction of every channel's RDS blocks (fmr_set_rds_correction), at any time after enable_rds()
  void set_rds_correction(int mode, int max_burst = 0, int soft_symbols = 0, double soft_max_cost = 0.0) {
    fmr_detail::rds_correction(m_chain, mode, max_burst, soft_symbols, soft_max_cost);
  }
  std::vector<fmr_rds_group> get_rds_groups(size_t ch) {
    if (ch >= m_offsets.size() || m_stations.empty()) fmr_detail::fail("ChannelBank: no RDS on this channel (enable_rds)");
    return fmr_detail::rds_groups(m_chain, (int)ch, m_stations[ch]);
  }
  const fmr_rds::Station &rds_station(size_t ch) { get_rds_groups(ch); return m_stations[ch]; }

  // Modulation monitor of every channel (fmr_enable_monitor), before the first process(), once; FM banks only.
  // read_modulation_records(ch) drains channel ch's complete records, oldest first.
  void enable_modulation_monitor(uint32_t interval_samples = 0, int hist_bins = 0, double hist_range = 0.0, int max_records = 0) {
    m_stages.monitor(m_chain, interval_samples, hist_bins, hist_range, max_records);
  }
  std::vector<ModulationRecord> read_modulation_records(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::monitor_records(m_chain, (int)ch);
  }
  // Audio monitor of every channel (fmr_enable_loudness), before the first process(), once; FM banks only.
  // read_loudness(ch) drains channel ch's complete records and derives their levels.
  void enable_loudness(uint32_t step_samples = 0, int max_records = 0) {
    m_stages.loudness(m_chain, step_samples, max_records);
  }
  LoudnessReport read_loudness(size_t ch, double silence_dbfs = -60.0) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::loudness_report(m_chain, (int)ch, silence_dbfs);
  }
  // Weak-signal handling of every channel (fmr_enable_weak_signal), before the first process(), once; FM banks only.
  // read_weak_signal(ch) drains channel ch's complete records and pools them.
  void enable_weak_signal(fmr_weak_signal_config cfg = fmr_weak_signal_config{}) {
    m_stages.weak_signal(m_chain, cfg);
  }
  WeakSignalReport read_weak_signal(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::weak_signal_report(m_chain, (int)ch);
  }
  // Impulse blanker on the capture (fmr_enable_blanker), before the first process(), once: one row serves all channels.
  // read_blanker() drains the capture's complete records and pools them.
  void enable_blanker(fmr_blanker_config cfg = fmr_blanker_config{}) {
    m_stages.blanker(m_chain, cfg);
  }
  BlankerReport read_blanker() { return fmr_detail::blanker_report(m_chain, 0, m_cfg.input_rate); }
  // DC-offset and IQ-imbalance correction of the same input (fmr_enable_iq_correction), under the same rules as
  // enable_blanker() and before or after it: cfg holds the fields to set (zeros = the defaults; FMR_IQC_MEASURE records
  // only, FMR_IQC_ACT corrects what the blanker and the front end read).  read_iq_correction() drains the complete
  // records and pools them.
  void enable_iq_correction(fmr_iq_correction_config cfg = fmr_iq_correction_config{}) {
    m_stages.iq_correction(m_chain, cfg);
  }
  IqCorrectionReport read_iq_correction() { return fmr_detail::iq_correction_report(m_chain, 0); }

  // Audio analyser of every channel (fmr_enable_analyser), before the first process(), once.  read_analyser(ch) drains
  // channel ch's complete records and derives their pooled levels.
  void enable_analyser(int fft_size = 0, uint32_t interval_samples = 0, int max_records = 0) {
    m_stages.analyser(m_chain, fft_size, interval_samples, max_records);
  }
  AnalyserReport read_analyser(size_t ch, int view = 0, double tone_hz = 0.0) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::analyser_report(m_chain, (int)ch, m_stages.analyser_cfg(), fmr_detail::analyser_rule(view, tone_hz));
  }

  // RF monitor of every channel (fmr_enable_rf_monitor), before the first process(), once; FM banks only.
  // read_rf_records(ch) drains channel ch's complete records, oldest first.
  void enable_rf_monitor(uint32_t interval_samples = 0, int max_records = 0) {
    m_stages.rf_monitor(m_chain, interval_samples, max_records);
  }
  std::vector<RfRecord> read_rf_records(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::rf_records(m_chain, (int)ch);
  }

  // Output stage of every channel (fmr_enable_output), before the first process(), once; banks of every mode.
  // rate / mono: every channel's PCM ring at that rate and / or downmixed (fmr_set_output_rate).
  // read_output(ch) drains channel ch's PCM frames and block records.
  void enable_output(int format = FMR_PCM_S16, double squelch_level = 0.0, double gain = 0.0, uint32_t max_frames = 0,
                     uint32_t max_blocks = 0, int rate = 0, bool mono = false) {
    m_stages.output(m_chain, fmr_detail::output_config(format, squelch_level, gain, max_frames, max_blocks),
                    fmr_detail::output_rate_config(rate, mono));
  }
  OutputData read_output(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::output_data(m_chain, (int)ch);
  }
  fmr_output_rate_info output_rate_info(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::output_rate_info(m_chain, (int)ch);
  }
  // MPX output of every channel (fmr_enable_mpx_output), before the first process(), once; FM banks only.
  // read_mpx_output(ch) drains channel ch's composite baseband as mono PCM at `rate`.
  void enable_mpx_output(int format = FMR_PCM_S16, int rate = 192000, double gain = 0.0, uint32_t max_frames = 0) {
    m_stages.mpx_output(m_chain, fmr_detail::mpx_output_config(format, rate, gain, max_frames));
  }
  MpxOutputData read_mpx_output(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    return fmr_detail::mpx_output_data(m_chain, (int)ch);
  }

  // audio[k] = what channel k produced from this capture block (empty = "nothing yet"); blocks longer than the chain's
  // block capacity are decoded in consecutive pieces
  void process(const IQSampleVector &samples_in, std::vector<SampleVector> &audio) {
    const size_t K = m_offsets.size();
    audio.assign(K, SampleVector());
    std::vector<double> buf;
    for (size_t off = 0; off < samples_in.size(); off += m_max_block) {
      const size_t n = std::min(m_max_block, samples_in.size() - off);
      const size_t stride = 2 * (n + 64);
      buf.assign(K * stride, 0.0);
      uint32_t bl = (uint32_t)n, al = 0;
      fmr_detail::check(fmr_process_blocks(m_chain, reinterpret_cast<const float *>(samples_in.data() + off), n, &bl, 1,
                                           buf.data(), stride, &al),
                        "fmr_process_blocks");
      for (size_t k = 0; k < K; k++) audio[k].insert(audio[k].end(), buf.begin() + k * stride, buf.begin() + k * stride + al);
    }
  }
  bool stereo_detected(size_t ch) { return status(ch).stereo_detected != 0; }
  float get_tuning_offset(size_t ch) {     // FmDecoder: x 75 kHz; NbfmDecoder: x its freq_dev
    return (float)(status(ch).baseband_mean * m_freq_dev);
  }
  float get_baseband_level(size_t ch) { return status(ch).baseband_level; }
  double get_pilot_level(size_t ch) { return status(ch).pilot_level; }
  float get_if_rms(size_t ch) { return status(ch).if_rms; }
  float get_if_agc_gain(size_t ch) { return status(ch).if_agc_gain; }
  double get_multipath_error(size_t ch) { return status(ch).multipath_error; }
  // PPS events of channel ch in the most recent process() call
  std::vector<PilotPhaseLock::PpsEvent> get_pps_events(size_t ch) {
    status(ch);
    fmr_pps_event ev[64];
    const int n = fmr_get_pps_events(m_chain, (int)ch, ev, 64);
    std::vector<PilotPhaseLock::PpsEvent> out;
    for (int i = 0; i < n && i < 64; i++) out.push_back({ev[i].pps_index, ev[i].sample_index, ev[i].block_position});
    return out;
  }

private:
  fmr_status status(size_t ch) {
    if (ch >= m_offsets.size()) fmr_detail::fail("ChannelBank: channel index out of range");
    fmr_status st{};
    fmr_detail::check(fmr_get_status(m_chain, (int)ch, &st), "fmr_get_status");
    return st;
  }
  std::vector<int32_t> m_offsets;
  size_t m_max_block;
  double m_freq_dev;
  fmr_config m_cfg{};
  std::vector<fmr_rds::Station> m_stations;
  fmr_detail::Stages m_stages;
  fmr_chain *m_chain = nullptr;
};

// Channelizer (fmr_create_channelizer): the IfResampler of several stations out of one wideband capture -- channel k is
// IfResampler(input_rate, output_rate) (IfResampler.h:35-38) of the capture shifted down by offsets_hz[k], the station
// at +offsets_hz[k] Hz.  Same default class as IfResampler and ChannelBank.  process() takes the capture block once and
// returns one IQ vector per channel at output_rate, e.g. for fmr_io::IqFileWriter or a decoder of the caller's own.
class Channelizer {
public:
  Channelizer(double input_rate, const std::vector<int32_t> &offsets_hz, double output_rate = 384000,
              int resampler_class = FMR_RESAMPLER_R8B, int device = 0, size_t max_block_len = 65536)
      : m_offsets(offsets_hz), m_max_block(max_block_len) {
    if (m_offsets.empty()) fmr_detail::fail("Channelizer: no channel");
    fmr_config cfg{};
    cfg.device = device; cfg.n_streams = (int)m_offsets.size(); cfg.mode = -1; cfg.input_rate = input_rate;
    cfg.output_rate = output_rate; cfg.enable_resampler = 1; cfg.resampler_class = resampler_class;
    cfg.max_block_len = max_block_len; cfg.max_blocks = 1; cfg.channel_offset_hz = m_offsets.data();
    fmr_detail::check(fmr_create_channelizer(&cfg, sizeof cfg, &m_chain), "fmr_create_channelizer");
    m_rate = input_rate;
  }
  ~Channelizer() { fmr_destroy(m_chain); }
  Channelizer(const Channelizer &) = delete;
  Channelizer &operator=(const Channelizer &) = delete;

  size_t channels() const { return m_offsets.size(); }
  int32_t offset_hz(size_t ch) const { return m_offsets.at(ch); }

  // Impulse blanker on the capture (fmr_enable_blanker), before the first process(), once: one row serves all channels.
  // read_blanker() drains the capture's complete records and pools them.
  void enable_blanker(fmr_blanker_config cfg = fmr_blanker_config{}) {
    m_stages.blanker(m_chain, cfg);
  }
  BlankerReport read_blanker() { return fmr_detail::blanker_report(m_chain, 0, m_rate); }
  // DC-offset and IQ-imbalance correction of the same input (fmr_enable_iq_correction), under the same rules as
  // enable_blanker() and before or after it: cfg holds the fields to set (zeros = the defaults; FMR_IQC_MEASURE records
  // only, FMR_IQC_ACT corrects what the blanker and the front end read).  read_iq_correction() drains the complete
  // records and pools them.
  void enable_iq_correction(fmr_iq_correction_config cfg = fmr_iq_correction_config{}) {
    m_stages.iq_correction(m_chain, cfg);
  }
  IqCorrectionReport read_iq_correction() { return fmr_detail::iq_correction_report(m_chain, 0); }

  // out[k] = what channel k produced from this capture block; blocks longer than the chain's block capacity are
  // resampled in consecutive pieces
  void process(const IQSampleVector &in, std::vector<IQSampleVector> &out) {
    const size_t K = m_offsets.size();
    out.assign(K, IQSampleVector());
    IQSampleVector buf;
    for (size_t off = 0; off < in.size(); off += m_max_block) {
      const size_t n = std::min(m_max_block, in.size() - off);
      const size_t stride = n + 64;
      buf.assign(K * stride, IQSample());
      uint32_t bl = (uint32_t)n, ol = 0;
      fmr_detail::check(fmr_resample_blocks(m_chain, reinterpret_cast<const float *>(in.data() + off), n, &bl, 1,
                                            reinterpret_cast<float *>(buf.data()), stride, &ol),
                        "fmr_resample_blocks");
      for (size_t k = 0; k < K; k++) out[k].insert(out[k].end(), buf.begin() + k * stride, buf.begin() + k * stride + ol);
    }
  }

private:
  std::vector<int32_t> m_offsets;
  size_t m_max_block;
  double m_rate = 0.0;
  fmr_chain *m_chain = nullptr;
  fmr_detail::Stages m_stages;
};

// SpectrumMonitor (fmr_spectrum_*): the Welch power spectrum of a capture on the GPU (mean PSD, density-scaled, fftshift
// order: element k is the bin at (k - N/2) input_rate / N Hz) and the stations it holds.  find_stations() returns offsets
// that go straight into ChannelBank / Channelizer.  Blocks longer than max_call_len are taken in consecutive pieces.
// The second constructor adds a waterfall (fmr_spectrum_create_waterfall): one line per waterfall_segments segments,
// waterfall_lines of them kept until read_waterfall() takes them.
class SpectrumMonitor {
public:
  explicit SpectrumMonitor(double input_rate, int fft_size = 8192, int hop = 0, int window = FMR_WINDOW_HANN, int device = 0,
                           size_t max_call_len = 1 << 20)
      : m_rate(input_rate), m_n(fft_size), m_max(max_call_len) {
    fmr_spectrum_config cfg{};
    cfg.struct_size = sizeof cfg; cfg.device = device; cfg.n_rows = 1; cfg.input_rate = input_rate;
    cfg.input_format = FMR_IQ_CF32; cfg.fft_size = fft_size; cfg.hop = hop; cfg.window = window; cfg.max_call_len = max_call_len;
    fmr_detail::check(fmr_spectrum_create(&cfg, sizeof cfg, &m_s), "fmr_spectrum_create");
  }
  SpectrumMonitor(double input_rate, int fft_size, int hop, int window, int device, size_t max_call_len,
                  int waterfall_segments, int waterfall_lines, int waterfall_which = FMR_WATERFALL_MEAN)
      : m_rate(input_rate), m_n(fft_size), m_max(max_call_len) {
    fmr_spectrum_config cfg{};
    cfg.struct_size = sizeof cfg; cfg.device = device; cfg.n_rows = 1; cfg.input_rate = input_rate;
    cfg.input_format = FMR_IQ_CF32; cfg.fft_size = fft_size; cfg.hop = hop; cfg.window = window; cfg.max_call_len = max_call_len;
    fmr_waterfall_config wf{};
    wf.struct_size = sizeof wf; wf.segments_per_line = waterfall_segments; wf.max_lines = waterfall_lines; wf.which = waterfall_which;
    fmr_detail::check(fmr_spectrum_create_waterfall(&cfg, sizeof cfg, &wf, sizeof wf, &m_s), "fmr_spectrum_create_waterfall");
  }
  ~SpectrumMonitor() { fmr_spectrum_destroy(m_s); }
  SpectrumMonitor(const SpectrumMonitor &) = delete;
  SpectrumMonitor &operator=(const SpectrumMonitor &) = delete;

  void process(const IQSampleVector &samples_in) {
    for (size_t off = 0; off < samples_in.size(); off += m_max) {
      const size_t n = std::min(m_max, samples_in.size() - off);
      fmr_detail::check(fmr_spectrum_process(m_s, samples_in.data() + off, n, n), "fmr_spectrum_process");
    }
  }
  // the mean PSD since construction / reset()
  std::vector<double> psd() { return read(0); }
  std::vector<double> peak_hold() { return read(1); }
  void reset() { fmr_detail::check(fmr_spectrum_reset(m_s), "fmr_spectrum_reset"); }
  // Every complete waterfall line not read yet (row 0 is the monitor's only row): lines.size() / fft_size lines of
  // fft_size floats in fftshift order, their counted segments in `counted`.  Returns the first line's absolute index.
  uint64_t read_waterfall(int row, std::vector<float> &lines, std::vector<uint32_t> &counted) {
    fmr_waterfall_info info{};
    const int ready = fmr_spectrum_read_waterfall(m_s, row, nullptr, nullptr, 0, &info);
    if (ready < 0) fmr_detail::check(ready, "fmr_spectrum_read_waterfall");
    lines.assign((size_t)ready * (size_t)m_n, 0.f);
    counted.assign((size_t)ready, 0);
    if (ready > 0) {
      const int rc = fmr_spectrum_read_waterfall(m_s, row, lines.data(), counted.data(), (size_t)ready, &info);
      if (rc < 0) fmr_detail::check(rc, "fmr_spectrum_read_waterfall");
    }
    return info.first_line;
  }
  // fmr_find_stations on the current mean PSD: offsets in ascending order
  std::vector<int32_t> find_stations(const fmr_station_rule &rule) {
    const std::vector<double> p = psd();
    const int n = fmr_find_stations(p.data(), m_n, m_rate, &rule, nullptr, 0);
    if (n < 0) fmr_detail::check(n, "fmr_find_stations");
    std::vector<fmr_station> st((size_t)n);
    fmr_find_stations(p.data(), m_n, m_rate, &rule, st.data(), n);
    std::vector<int32_t> out;
    for (const fmr_station &x : st) out.push_back(x.offset_hz);
    return out;
  }

private:
  std::vector<double> read(int which) {
    std::vector<double> v((size_t)m_n);
    const int rc = fmr_spectrum_read(m_s, 0, which, v.data(), v.size(), nullptr);
    if (rc < 0) fmr_detail::check(rc, "fmr_spectrum_read");
    return v;
  }
  double m_rate;
  int m_n;
  size_t m_max;
  fmr_spectrum *m_s = nullptr;
};
