// Drives the library's RDS data link layer (host/fmradion_rds.hpp) on a bit file, for tests/test_rds_host.py.
//   rds_sync_check BITS [INDEX [hold]]   BITS: one byte (0 / 1) per data bit; INDEX: one uint64 sample index per bit ("-":
//   i); hold: the queue is drained only at the end (the reader that never drains)
// Prints "G sample_index b0 b1 b2 b3 s0 s1 s2 s3" per group and "S synced blocks_ok blocks_bad decoded dropped" at the end.
#include <cstdio>
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
  if (argc < 2) return 2;
  const std::vector<unsigned char> bits = slurp(argv[1]);
  const std::vector<unsigned char> raw = argc > 2 ? slurp(argv[2]) : std::vector<unsigned char>();
  const bool hold = argc > 3;
  fmr_rds::Decoder d;
  fmr_rds_group g[64];
  auto flush = [&] {
    for (size_t n; (n = d.pop(g, 64)) > 0;)
      for (size_t i = 0; i < n; i++)
        std::printf("G %llu %u %u %u %u %u %u %u %u\n", (unsigned long long)g[i].sample_index, g[i].block[0], g[i].block[1],
                    g[i].block[2], g[i].block[3], g[i].status[0], g[i].status[1], g[i].status[2], g[i].status[3]);
  };
  for (size_t i = 0; i < bits.size(); i++) {
    unsigned long long idx = i;
    if (raw.size() >= 8 * (i + 1)) {
      idx = 0;
      for (int b = 7; b >= 0; b--) idx = (idx << 8) | raw[8 * i + b];
    }
    d.push(bits[i], idx);
    if (!hold && d.queued() >= 32) flush();
  }
  flush();
  std::printf("S %d %llu %llu %llu %llu\n", (int)d.synced(), (unsigned long long)d.blocks_ok(),
              (unsigned long long)d.blocks_bad(), (unsigned long long)d.groups_decoded(),
              (unsigned long long)d.groups_dropped());
  return 0;
}
