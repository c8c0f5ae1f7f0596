// MPX output through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz with the composite at 192 kHz S16, and a
// two-channel ChannelBank at 2.5 MS/s with the composite at 171 kHz F32.  Every stream's ring must hold ceil(F L / M) frames
// for the F MPX samples it took, with the geometry of fmr_mpx_output_taps and nothing dropped; the decoder's station is a
// 1 kHz tone at 37.5 kHz deviation, so at gain 0.5 its S16 composite must peak near 0.25 x 32767.  The FM stream's frames
// then go to a 192 kHz mono WAV file through AudioFileWriter (argv[1]).  Prints "<name> frames N of F rate R" per stream and
// "wav bytes B"; exit status 0 when all of it holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "fmradion_facade.hpp"
#include "fmradion_fileio.hpp"

// FM of a 1 kHz tone at +f Hz: deviation dev Hz, carrier amplitude amp
static void add_station(IQSampleVector &x, double fs, double amp, long long f, double dev) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * dev / fs * std::sin(2 * M_PI * 1000.0 * (n / fs));
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

static bool report(const char *name, const MpxOutputData &o, int rate, int format) {
  int L = 0, M = 0, T = 0;
  bool ok = fmr_mpx_output_taps(rate, nullptr, 0, &L, &M, &T) == L * T;
  const uint64_t F = o.info.samples_in, want = (F * (uint64_t)L + (uint64_t)M - 1) / (uint64_t)M;
  ok = ok && F > 0 && o.info.rate == rate && o.info.format == format && o.info.L == L && o.info.M == M &&
       o.info.taps_per_phase == T && o.info.delay_frames == ((double)T * L - 1.0) / (2.0 * M) && o.info.full_scale_hz == 150000.0;
  ok = ok && o.frames == want && o.info.first_frame == 0 && o.info.frames_waiting == 0 && o.info.frames_dropped == 0 &&
       o.info.pcm_clipped == 0 && o.info.pcm_nonfinite == 0;
  std::printf("%s frames %zu of %llu rate %d\n", name, o.frames, (unsigned long long)F, o.info.rate);
  return ok;
}

int main(int argc, char **argv) {
  bool ok = true;
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  {
    const double fs = 384000.0;
    IQSampleVector x((size_t)(0.25 * fs));
    add_station(x, fs, 0.3, 0, 37500.0);
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_mpx_output(FMR_PCM_S16, 192000);
    SampleVector audio;
    for (size_t off = 0; off < x.size(); off += 20000)
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 20000)), audio);
    const MpxOutputData o = fm.read_mpx_output();
    ok = report("fm", o, 192000, FMR_PCM_S16) && o.info.samples_in == x.size() && ok;
    int peak = 0;
    for (size_t m = o.frames / 2; m < o.frames; m++) peak = std::max(peak, std::abs((int)o.s16()[m]));
    std::printf("fm peak %d\n", peak);
    ok = ok && peak > 7900 && peak < 8500;       // 0.5 x 37.5 / 75 x 32767 = 8192
    if (argc > 1) {
      fmr_io::AudioFileWriter w;
      ok = w.open(argv[1], 192000, false, fmr_io::AudioFormat::WAV_INT16) && w.write_i16(o.s16(), o.frames) && ok;
      w.close();
      FILE *f = std::fopen(argv[1], "rb");
      long bytes = 0;
      if (f) { std::fseek(f, 0, SEEK_END); bytes = std::ftell(f); std::fclose(f); }
      std::printf("wav bytes %ld\n", bytes);
      ok = ok && bytes > (long)(2 * o.frames);
    }
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(0.1 * fs));
    add_station(x, fs, 0.3, -600000, 37500.0);
    add_station(x, fs, 0.2, 500000, 37500.0);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_mpx_output(FMR_PCM_F32, 171000);
    std::vector<SampleVector> audio;
    for (size_t off = 0; off < x.size(); off += 65536)
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
    for (int k = 0; k < 2; k++) {
      const MpxOutputData o = bank.read_mpx_output((size_t)k);
      ok = report(k ? "bank1" : "bank0", o, 171000, FMR_PCM_F32) && ok;
      float peak = 0.f;
      for (size_t m = o.frames / 2; m < o.frames; m++) peak = std::max(peak, std::fabs(o.f32()[m]));
      ok = ok && peak > 0.24f && peak < 0.26f;
    }
  }
  return ok ? 0 : 1;
}
