// Output stage at other rates through the facade (host/fmradion_facade.hpp): an FmDecoder at 384 kHz with 16 kHz mono F32
// PCM, an NbfmDecoder at 48 kHz with 8 kHz S16 PCM (squelched: the carrier is under the level) and a two-channel
// ChannelBank at 2.5 MS/s with 44.1 kHz stereo S16 PCM (one station open, one squelched).  Every open stream's PCM must be
// the definition of the header evaluated here on the audio process() returned, with the taps of fmr_output_rate_taps;
// every squelched one's all zero; the block records still count the decoder's frames.  The FM stream's PCM then goes to a
// 16 kHz mono WAV file through AudioFileWriter (argv[1]).  Prints "<name> frames N of M rate R" per stream and
// "wav bytes B"; exit status 0 when all of it holds.
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

// audio: the decoder's doubles (in_ch interleaved); the ring has out_ch channels
static bool report(const char *name, const OutputData &o, const fmr_output_rate_info &ri, const SampleVector &audio, int in_ch,
                   int out_ch, int rate, bool f32, bool open) {
  int L = 0, M = 0, T = 0;
  const int n = fmr_output_rate_taps(rate, nullptr, 0, &L, &M, &T);
  std::vector<double> h((size_t)(n > 0 ? n : 0));
  bool ok = n > 0 && fmr_output_rate_taps(rate, h.data(), n, nullptr, nullptr, nullptr) == n;
  const size_t F = audio.size() / (size_t)in_ch, want = (F * (size_t)L + (size_t)M - 1) / (size_t)M;
  ok = ok && ri.rate == rate && ri.channels == out_ch && ri.L == L && ri.M == M && ri.taps_per_phase == T && ri.frames_in == F &&
       ri.pcm_nonfinite == 0 && ri.delay_frames == ((double)T * L - 1.0) / (2.0 * M);
  ok = ok && o.info.channels == out_ch && o.info.frames_waiting == 0 && o.info.frames_dropped == 0 && o.info.first_frame == 0 &&
       o.frames == want;
  uint64_t frame = 0;
  for (const fmr_output_block &b : o.blocks) {
    ok = ok && b.first_frame == frame && b.channels == (uint32_t)in_ch && b.gate_open == (open ? 1u : 0u);
    frame += b.n_frames;
  }
  ok = ok && frame == F;
  const double g = open ? 0.5 : 0.0;
  for (size_t m = 0; ok && m < o.frames; m++) {
    const long long q = (long long)(m * (size_t)M / (size_t)L);
    const int p = (int)(m * (size_t)M % (size_t)L);
    for (int c = 0; c < out_ch; c++) {
      volatile double acc = 0.0;      // (volatile: every product and sum rounded by itself, whatever the host compiler fuses)
      for (int k = 0; k < T && q - k >= 0; k++) {
        const size_t j = (size_t)(q - k);
        const double x = in_ch == out_ch ? audio[j * in_ch + c] : (audio[2 * j] + audio[2 * j + 1]) * 0.5;
        volatile double pr = h[(size_t)k * L + p] * (x * g);
        acc = acc + pr;
      }
      const double y = acc;
      ok = f32 ? o.f32()[m * out_ch + c] == (float)y : o.s16()[m * out_ch + c] == (int16_t)std::lrint(y * 32767.0);
    }
  }
  std::printf("%s frames %zu of %zu rate %d\n", name, o.frames, F, ri.rate);
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
    fm.enable_output(FMR_PCM_F32, level, 0.0, 0, 0, 16000, true);
    SampleVector audio, all;
    for (size_t off = 0; off < x.size(); off += 20000) {
      fm.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 20000)), audio);
      all.insert(all.end(), audio.begin(), audio.end());
    }
    const OutputData o = fm.read_output();
    ok = report("fm", o, fm.output_rate_info(), all, 2, 1, 16000, true, true) && ok;
    if (argc > 1) {
      fmr_io::AudioFileWriter w;
      ok = w.open(argv[1], 16000, false, fmr_io::AudioFormat::WAV_FLOAT32) && w.write_f32(o.f32(), o.samples()) && ok;
      w.close();
      FILE *f = std::fopen(argv[1], "rb");
      long bytes = 0;
      if (f) { std::fseek(f, 0, SEEK_END); bytes = std::ftell(f); std::fclose(f); }
      std::printf("wav bytes %ld\n", bytes);
      ok = ok && bytes > (long)(4 * o.samples());
    }
  }
  {
    const double fs = 48000.0;
    IQSampleVector x(16 * 2048);
    add_station(x, fs, 0.003, 0, 3000.0);
    IQSampleCoeff coeff = FilterParameters::iq("jj1bdx_nbfm_48khz_default");
    NbfmDecoder nb(coeff, NbfmDecoder::freq_dev_normal);
    nb.enable_output(FMR_PCM_S16, level, 0.0, 0, 0, 8000);
    SampleVector audio, all;
    for (size_t off = 0; off < x.size(); off += 2048) {
      nb.process(IQSampleVector(x.begin() + off, x.begin() + off + 2048), audio);
      all.insert(all.end(), audio.begin(), audio.end());
    }
    ok = report("nbfm", nb.read_output(), nb.output_rate_info(), all, 1, 1, 8000, false, false) && ok;
  }
  {
    const double fs = 2.5e6;
    IQSampleVector x((size_t)(0.2 * fs));
    add_station(x, fs, 0.3, -600000, 37500.0);
    add_station(x, fs, 0.003, 500000, 37500.0);
    ChannelBank bank(fs, {-600000, 500000}, ModType::FM, false, delay, true, FmDecoder::deemphasis_time_eu, false, 0);
    bank.enable_output(FMR_PCM_S16, level, 0.0, 0, 0, 44100);
    std::vector<SampleVector> audio, all(2);
    for (size_t off = 0; off < x.size(); off += 65536) {
      bank.process(IQSampleVector(x.begin() + off, x.begin() + std::min(x.size(), off + 65536)), audio);
      for (int k = 0; k < 2; k++) all[k].insert(all[k].end(), audio[k].begin(), audio[k].end());
    }
    ok = report("bank0", bank.read_output(0), bank.output_rate_info(0), all[0], 2, 2, 44100, false, true) && ok;
    ok = report("bank1", bank.read_output(1), bank.output_rate_info(1), all[1], 2, 2, 44100, false, false) && ok;
  }
  return ok ? 0 : 1;
}
