// MPX input through the facade (host/fmradion_facade.hpp, host/fmradion_fileio.hpp): an FmDecoder at 384 kHz archives its
// composite at 192 kHz S16 into a mono WAV file (argv[1]) through AudioFileWriter; MpxFileReader reads the file back --
// rate, format and frames -- and an MpxDecoder decodes it.  The station is a 1 kHz tone at 37.5 kHz deviation.  Checked:
// the reader reports 192000 / int16 and delivers every frame written; the decoder took them all and made
// ceil(F M / L) = 2 F MPX samples of them (the count law), in blocks of the MPX counts the IQ decoder was fed, so the audio
// has the IQ decoder's length, sample for sample; it is finite and carries the tone (its peak lies near the IQ decoder's).
// Prints the figures and "OK"; exit status 0 when all of it holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "fmradion_facade.hpp"
#include "fmradion_fileio.hpp"

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: mpx_input_smoke FILE.wav\n"); return 2; }
  bool ok = true;
  const double fs = 384000.0;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  size_t written = 0, total_iq = 0;
  double peak_iq = 0.0;
  {
    IQSampleVector x((size_t)(0.25 * fs));
    double ph = 0.0;
    for (size_t n = 0; n < x.size(); n++) {
      ph += 2 * M_PI * 37500.0 / fs * std::sin(2 * M_PI * 1000.0 * (n / fs));
      x[n] = IQSample((float)(0.3 * std::cos(ph)), (float)(0.3 * std::sin(ph)));
    }
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_mpx_output(FMR_PCM_S16, 192000);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 20000) {
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 20000)), audio);
      total_iq += audio.size();
      if (off >= x.size() / 2) for (double v : audio) peak_iq = std::max(peak_iq, std::fabs(v));
    }
    const MpxOutputData o = fm.read_mpx_output();
    fmr_io::AudioFileWriter w;
    ok = w.open(argv[1], 192000, false, fmr_io::AudioFormat::WAV_INT16) && w.write_i16(o.s16(), o.frames) && ok;
    w.close();
    written = o.frames;
    ok = ok && written == x.size() / 2;
  }
  fmr_io::MpxFileReader r;
  if (!r.open(argv[1])) { std::fprintf(stderr, "MpxFileReader: %s\n", r.error().c_str()); return 1; }
  std::printf("file rate %u float %d\n", r.sample_rate(), (int)r.is_float());
  ok = ok && r.sample_rate() == 192000 && !r.is_float();
  MpxDecoder dec((int)r.sample_rate(), r.is_float() ? FMR_PCM_F32 : FMR_PCM_S16, true);
  std::vector<int16_t> frames;
  std::vector<float> none;
  ok = ok && !r.read_f32(none, 16);
  SampleVector audio;
  size_t total = 0, read = 0;
  double peak = 0.0;
  bool finite = true;
  while (r.read_i16(frames, 10000)) {
    read += frames.size();
    dec.process(frames, audio);
    total += audio.size();
    for (double v : audio) finite = finite && std::isfinite(v);
    if (read >= written / 2) for (double v : audio) peak = std::max(peak, std::fabs(v));
  }
  const fmr_mpx_input_info i = dec.input_info();
  std::printf("frames %zu of %zu, MPX samples %llu, audio %zu (IQ decoder %zu), peak %.4f (IQ decoder %.4f)\n", read, written,
              (unsigned long long)i.samples_out, total, total_iq, peak, peak_iq);
  ok = ok && read == written && i.frames_in == written && i.samples_out == 2 * (uint64_t)written && i.rate == 192000 &&
       i.L == 1 && i.M == 2 && i.taps_per_sample == 143 && i.full_scale_hz == 150000.0 && i.nonfinite_in == 0;
  ok = ok && finite && total % 2 == 0 && total > 0 && total == total_iq;
  ok = ok && peak > 0.0 && std::fabs(peak - peak_iq) <= 0.02 * peak_iq;
  if (ok) std::printf("OK\n");
  return ok ? 0 : 1;
}
