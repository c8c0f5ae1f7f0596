// AudioFileWriter::write_i16 (host/fmradion_fileio.hpp): int16 samples from a file into a RAW / WAV container as they
// are, in ragged pieces; tests/test_output_args.py reads the container back (IqFileReader for the stereo WAV).
//   output_fileio_check write <RAW_INT16|WAV_INT16|WAV_FLOAT32> <in.s16> <out> <rate> <stereo> <piece>
//   output_fileio_check read  <in.wav> <out.cf32>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../airspy-fmradion_amd/host/fmradion_fileio.hpp"

using namespace fmr_io;

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "write" && argc == 8) {
    const std::string f = argv[2];
    const AudioFormat fmt = f == "RAW_INT16" ? AudioFormat::RAW_INT16 : f == "WAV_INT16" ? AudioFormat::WAV_INT16 : AudioFormat::WAV_FLOAT32;
    FILE *fi = fopen(argv[3], "rb");
    if (!fi) return 3;
    std::vector<int16_t> v;
    int16_t buf[4096];
    for (size_t n; (n = fread(buf, 2, 4096, fi)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(fi);
    AudioFileWriter w;
    if (!w.open(argv[4], (unsigned)atoi(argv[5]), atoi(argv[6]) != 0, fmt)) { std::printf("error: %s\n", w.error().c_str()); return 3; }
    const size_t piece = (size_t)atol(argv[7]);
    size_t pos = 0, refused = 0;
    while (pos < v.size()) {
      const size_t n = std::min(piece, v.size() - pos);
      if (!w.write_i16(v.data() + pos, n)) { refused++; break; }
      pos += n;
    }
    if (!w.write_i16(nullptr, 0) && !refused) refused++;      // an empty write is fine on an int16 container
    w.close();
    std::printf("written %zu refused %zu\n", pos, refused);
    return 0;
  }
  if (cmd == "read" && argc == 4) {
    IqFileReader r;
    if (!r.open(argv[2], false)) { std::printf("error: %s\n", r.error().c_str()); return 3; }
    FILE *fo = fopen(argv[3], "wb");
    if (!fo) return 3;
    IQSampleVector blk;
    size_t total = 0;
    while (r.read_block(blk, 1000)) { fwrite(blk.data(), sizeof(IQSample), blk.size(), fo); total += blk.size(); }
    fclose(fo);
    std::printf("rate %u samples %zu\n", (unsigned)r.sample_rate(), total);
    return 0;
  }
  return 2;
}
