// Output stage through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz (S16, open), an NbfmDecoder at 48 kHz
// (S16, squelched: the carrier is under the level), an AmDecoder at 48 kHz (F32, open) and a two-channel ChannelBank at
// 2.5 MS/s with one strong and one weak station (one open, one squelched).  Every open stream's PCM must be the audio
// process() returned times 0.5, converted as AudioFileWriter converts it; every squelched one's all zero; the records
// consecutive.  The FM stream's PCM then goes to a WAV file through AudioFileWriter::write_i16 (argv[1]).  Prints
// "<name> frames N blocks M open K" per stream and "wav bytes B"; exit status 0 when all of it holds.
#include <cmath>
#include <cstdio>

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

static bool report(const char *name, const OutputData &o, const SampleVector &audio, int channels, bool f32, bool open,
                   size_t min_blocks) {
  size_t n_open = 0;
  bool ok = o.info.channels == channels && o.info.format == (f32 ? FMR_PCM_F32 : FMR_PCM_S16) && o.info.frames_waiting == 0 &&
            o.info.blocks_waiting == 0 && o.info.frames_dropped == 0 && o.info.blocks_dropped == 0 && o.info.first_frame == 0;
  ok = ok && o.samples() == audio.size() && o.blocks.size() >= min_blocks;
  uint64_t frame = 0;
  for (size_t i = 0; i < o.blocks.size(); i++) {
    const fmr_output_block &b = o.blocks[i];
    ok = ok && b.block == i && b.first_frame == frame && b.channels == (uint32_t)channels && b.n_nonfinite == 0 && b.if_level > 0.f;
    frame += b.n_frames;
    n_open += b.gate_open;
  }
  ok = ok && frame == o.frames && n_open == (open ? o.blocks.size() : 0);
  for (size_t i = 0; ok && i < audio.size(); i++) {
    const double y = audio[i] * (open ? 0.5 : 0.0);
    ok = f32 ? o.f32()[i] == (float)y : o.s16()[i] == (int16_t)std::lrint(y * 32767.0);
  }
  std::printf("%s frames %zu blocks %zu open %zu\n", name, o.frames, o.blocks.size(), n_open);
  return ok;
}

int main(int argc, char **argv) {
  bool ok = true;
  const double level = fmr_squelch_level_from_db(30.0);      // 0.0316
  IQSampleCoeff delay{0.f, 1.f, 0.f};
  {
    const double fs = 384000.0;
    IQSampleVector x((size_t)(0.25 * fs));
    add_station(x, fs, 0.3, 0, 37500.0);
    FmDecoder fm(false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    fm.enable_output(FMR_PCM_S16, level);
    SampleVector audio, all;
    for (size_t off = 0; off < x.size(); off += 20000) {
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 20000)), audio);
      all.insert(all.end(), audio.begin(), audio.end());
    }
    const OutputData o = fm.read_output();
    ok = report("fm", o, all, 2, false, true, 5) && ok;
    ok = fm.read_output().frames == 0 && ok;                  // drained
    if (argc > 1) {
      fmr_io::AudioFileWriter w;
      ok = w.open(argv[1], 48000, true, fmr_io::AudioFormat::WAV_INT16) && w.write_i16(o.s16(), o.samples()) && ok;
      w.close();
      FILE *f = std::fopen(argv[1], "rb");
      long bytes = 0;
      if (f) { std::fseek(f, 0, SEEK_END); bytes = std::ftell(f); std::fclose(f); }
      std::printf("wav bytes %ld\n", bytes);
      ok = ok && bytes > (long)(2 * o.samples());
    }
  }
  {
    const double fs = 48000.0;
    IQSampleVector x(16 * 2048);
    add_station(x, fs, 0.003, 0, 3000.0);
    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_nbfm_48khz_default");
    NbfmDecoder nb(coeff, NbfmDecoder::freq_dev_normal);
    nb.enable_output(FMR_PCM_S16, level);
    SampleVector audio, all;
    for (size_t off = 0; off < x.size(); off += 2048) {
      nb.process(IQSampleVector(x.begin() + off, x.begin() + off + 2048), audio);
      all.insert(all.end(), audio.begin(), audio.end());
    }
    ok = report("nbfm", nb.read_output(), all, 1, false, false, 16) && ok;
  }
  {
    const double fs = 48000.0;
    IQSampleVector x(16 * 2048);
    for (size_t n = 0; n < x.size(); n++) x[n] = IQSample((float)(0.2 * (1.0 + 0.5 * std::sin(2 * M_PI * 1000.0 * n / fs))), 0.f);
    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_am_48khz_narrow");
    AmDecoder am(coeff, ModType::AM);
    am.enable_output(FMR_PCM_F32, level);
    SampleVector audio, all;
    for (size_t off = 0; off < x.size(); off += 2048) {
      am.process(IQSampleVector(x.begin() + off, x.begin() + off + 2048), audio);
      all.insert(all.end(), audio.begin(), audio.end());
    }
    ok = report("am", am.read_output(), all, 1, true, true, 16) && ok;
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(0.2 * fs));
    add_station(x, fs, 0.3, -600000, 37500.0);
    add_station(x, fs, 0.003, 500000, 37500.0);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_output(FMR_PCM_S16, level);
    std::vector<SampleVector> audio, all(2);
    for (size_t off = 0; off < x.size(); off += 65536) {
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
      for (int k = 0; k < 2; k++) all[k].insert(all[k].end(), audio[k].begin(), audio[k].end());
    }
    ok = report("bank0", bank.read_output(0), all[0], 2, false, true, 7) && ok;
    ok = report("bank1", bank.read_output(1), all[1], 2, false, false, 7) && ok;
  }
  return ok ? 0 : 1;
}
