// Drives the error correction of the library's RDS data link layer (host/fmradion_rds.hpp) on a bit file, for
// tests/test_rds_fec_host.py.
//   rds_fec_check BITS REL MODE MAX_BURST SOFT_SYMBOLS SOFT_MAX_COST [SWITCH_AT MODE2]
//   BITS: one byte (0 / 1) per data bit.  REL: one float32 per bit, the reliability |rho| of the bit's symbol; a negative
//   value: the bit is pushed without reliability; "-": every bit is.  MODE: 0 off, 1 burst, 2 soft, set before the first
//   bit; SWITCH_AT MODE2: set_correction(MODE2) in front of bit SWITCH_AT.  The sample index of bit i is i.
// Prints "T distinct" (the burst table's syndromes are all different: 1 / 0), "G sample_index b0 b1 b2 b3 s0 s1 s2 s3" per
// group and "S synced blocks_ok blocks_corrected blocks_bad decoded dropped" at the end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fmradion_rds.hpp"

static std::vector<unsigned char> slurp(const char *path) {
  std::vector<unsigned char> v;
  if (FILE *f = std::fopen(path, "rb")) {
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc < 7) return 2;
  const std::vector<unsigned char> bits = slurp(argv[1]);
  std::vector<float> rel;
  if (std::strcmp(argv[2], "-") != 0) {
    const std::vector<unsigned char> raw = slurp(argv[2]);
    rel.resize(raw.size() / sizeof(float));
    std::memcpy(rel.data(), raw.data(), rel.size() * sizeof(float));
    if (rel.size() != bits.size()) return 2;
  }
  fmr_rds::Correction c;
  c.mode = std::atoi(argv[3]);
  c.max_burst = std::atoi(argv[4]);
  c.soft_symbols = std::atoi(argv[5]);
  c.soft_max_cost = std::atof(argv[6]);
  const long long switch_at = argc > 8 ? std::atoll(argv[7]) : -1;
  fmr_rds::Decoder d;
  if (!d.set_correction(c)) { std::printf("E set_correction\n"); return 3; }
  std::printf("T %d\n", (int)fmr_rds::burst_table().distinct);
  fmr_rds_group g[64];
  auto flush = [&] {
    for (size_t n; (n = d.pop(g, 64)) > 0;)
      for (size_t i = 0; i < n; i++)
        std::printf("G %llu %u %u %u %u %u %u %u %u\n", (unsigned long long)g[i].sample_index, g[i].block[0], g[i].block[1],
                    g[i].block[2], g[i].block[3], g[i].status[0], g[i].status[1], g[i].status[2], g[i].status[3]);
  };
  for (size_t i = 0; i < bits.size(); i++) {
    if ((long long)i == switch_at) {
      c.mode = std::atoi(argv[8]);
      if (!d.set_correction(c)) { std::printf("E set_correction\n"); return 3; }
    }
    if (!rel.empty() && rel[i] >= 0.f) d.push(bits[i], i, rel[i]);
    else d.push(bits[i], i);
    if (d.queued() >= 32) flush();
  }
  flush();
  std::printf("S %d %llu %llu %llu %llu %llu\n", (int)d.synced(), (unsigned long long)d.blocks_ok(),
              (unsigned long long)d.blocks_corrected(), (unsigned long long)d.blocks_bad(),
              (unsigned long long)d.groups_decoded(), (unsigned long long)d.groups_dropped());
  return 0;
}
