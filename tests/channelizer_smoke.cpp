// Channelizer through the facade (host/fmradion_facade.hpp) and the IQ file container (host/fmradion_fileio.hpp).
//   channelizer_smoke DIR            three FM stations in one 2.5 MS/s capture, one Channelizer, every channel written to
//                                    DIR/ch<k>.wav with IqFileWriter and read back; prints "channels 3" and the lengths.
//                                    Without a GPU the facade stops with "no HIP device".
//   channelizer_smoke DIR --fileio   IqFileWriter -> IqFileReader round trip (no GPU): bit-exact, and the file is a valid
//                                    2-channel float WAV after every write.  Prints "iq round trip ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "fmradion_facade.hpp"
#include "fmradion_fileio.hpp"

static bool same_bits(const IQSample &a, const IQSample &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// everything in the file at `path` as IqFileReader delivers it; false if it does not open as a 2-channel float WAV
static bool read_all(const std::string &path, unsigned rate, IQSampleVector &all) {
  fmr_io::IqFileReader r;
  if (!r.open(path, false)) { std::fprintf(stderr, "open: %s\n", r.error().c_str()); return false; }
  if (r.sample_rate() != rate || r.format() != fmr_io::IqFormat::FLOAT) { std::fprintf(stderr, "header: rate / format\n"); return false; }
  all.clear();
  IQSampleVector blk;
  while (r.read_block(blk, 4096)) all.insert(all.end(), blk.begin(), blk.end());
  return true;
}

static int fileio(const std::string &dir) {
  const std::string path = dir + "/iq.wav";
  const unsigned rate = 192000;
  IQSampleVector ref;
  const float specials[] = {0.f, -0.f, std::numeric_limits<float>::quiet_NaN(), -std::numeric_limits<float>::infinity(),
                            std::numeric_limits<float>::infinity(), std::numeric_limits<float>::denorm_min(),
                            std::numeric_limits<float>::max(), -1.f, 1.f};
  fmr_io::IqFileWriter w;
  if (!w.open(path, rate)) { std::fprintf(stderr, "%s\n", w.error().c_str()); return 1; }
  IQSampleVector got;
  // writes of many sizes: the header is refreshed every half second of samples in between
  const size_t sizes[] = {1, 0, 7, 4096, 65536, 30001, 12345, 100000, 3, 70000};
  unsigned seed = 1;
  for (size_t n : sizes) {
    IQSampleVector blk(n);
    for (size_t i = 0; i < n; i++) {
      seed = seed * 1664525u + 1013904223u;
      float re, im;
      const unsigned a = seed, b = seed * 2654435761u;
      std::memcpy(&re, &a, 4);            // any bit pattern, NaN payloads included
      std::memcpy(&im, &b, 4);
      if (i % 97 == 0) re = specials[(i / 97) % 9];
      blk[i] = IQSample(re, im);
    }
    if (!w.write(blk)) { std::fprintf(stderr, "write: %s\n", w.error().c_str()); return 1; }
    ref.insert(ref.end(), blk.begin(), blk.end());
    // a reader now (the writer killed here) sees a valid file that holds a prefix of what was written
    if (!read_all(path, rate, got)) return 1;
    if (got.size() > ref.size()) { std::fprintf(stderr, "reader saw more than was written\n"); return 1; }
    for (size_t i = 0; i < got.size(); i++)
      if (!same_bits(got[i], ref[i])) { std::fprintf(stderr, "sample %zu differs before close\n", i); return 1; }
  }
  w.close();
  if (!read_all(path, rate, got)) return 1;
  if (got.size() != ref.size()) { std::fprintf(stderr, "length %zu != %zu\n", got.size(), ref.size()); return 1; }
  for (size_t i = 0; i < ref.size(); i++)
    if (!same_bits(got[i], ref[i])) { std::fprintf(stderr, "sample %zu differs\n", i); return 1; }
  std::printf("iq round trip ok %zu\n", ref.size());
  return 0;
}

// an FM carrier at rate fs, 75 kHz deviation, a tone of 1000 + 10 id Hz, at +f Hz
static void add_station(IQSampleVector &x, double fs, int id, double amp, long long f) {
  double ph = 0.0;
  const long long F = (long long)fs;
  for (size_t n = 0; n < x.size(); n++) {
    ph += 2 * M_PI * 75000.0 / fs * std::sin(2 * M_PI * (1000.0 + 10 * id) * n / fs);
    const double mix = 2 * M_PI * (double)(((f % F + F) % F) * (long long)(n % F) % F) / fs;
    x[n] += IQSample((float)(amp * std::cos(ph + mix)), (float)(amp * std::sin(ph + mix)));
  }
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  if (argc > 2 && std::strcmp(argv[2], "--fileio") == 0) return fileio(dir);
  const double fs = 2.5e6;
  const std::vector<int32_t> offs{-700000, 0, 600000};
  IQSampleVector x((size_t)(0.3 * fs));
  add_station(x, fs, 3, 0.3, offs[0]);
  add_station(x, fs, 8, 0.15, offs[1]);
  add_station(x, fs, 12, 0.2, offs[2]);
  Channelizer cz(fs, offs);
  std::vector<fmr_io::IqFileWriter> files(offs.size());
  for (size_t k = 0; k < offs.size(); k++)
    if (!files[k].open(dir + "/ch" + std::to_string(k) + ".wav", 384000)) { std::fprintf(stderr, "open failed\n"); return 1; }
  std::vector<IQSampleVector> out;
  std::vector<size_t> total(offs.size(), 0);
  for (size_t off = 0; off < x.size(); off += 100000) {          // (longer than the chain's block capacity: cut in pieces)
    IQSampleVector blk(x.begin() + off, x.begin() + std::min(x.size(), off + 100000));
    cz.process(blk, out);
    for (size_t k = 0; k < offs.size(); k++) { files[k].write(out[k]); total[k] += out[k].size(); }
  }
  for (auto &f : files) f.close();
  for (size_t k = 0; k < offs.size(); k++) {
    IQSampleVector back;
    if (!read_all(dir + "/ch" + std::to_string(k) + ".wav", 384000, back) || back.size() != total[k]) return 1;
  }
  std::printf("channels %zu\nlength %zu %zu %zu\n", cz.channels(), total[0], total[1], total[2]);
  return total[0] > 0 && total[0] == total[1] && total[1] == total[2] ? 0 : 1;
}
