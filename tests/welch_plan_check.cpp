// csrc/welch_plan.hpp on the host, with the host compiler alone (no HIP): the launch planner against a brute-force
// enumeration of welch_sub, the sizing against the numbers recorded from the formulas it replaced
// (tests/golden/welch_sizing.txt, the path is argv[1]), and the window / twiddle tables bit for bit against the three
// expressions the stages used before they shared welch_tables.  Prints one line per part; exit status 0 only if all pass.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I airspy-fmradion_amd/csrc tests/welch_plan_check.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>

#include "welch_plan.hpp"

using namespace fmr;

static int fails = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (fails++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                               \
  } while (0)

// every start j in the first three records, every end up to four records on: the launches tile [j, j_hi) in order
static long long check_planner() {
  const int subs[] = {1, 4, 5, 8, 16, 32}, rmaxs[] = {1, 2, 3, 7, 128};
  long long launches = 0;
  for (int spr = 1; spr <= 40; spr++)
    for (int sub : subs)
      for (int rmax : rmaxs) {
        const int sb = (spr + sub - 1) / sub;
        for (long long j = 0; j < 3LL * spr; j++) {
          for (long long e = j - 1; e <= j; e++) {          // nothing left: no run, one record's blocks for the carry
            const WelchLaunch p = welch_plan(spr, sub, sb, rmax, j, e);
            CHECK(p.runs == 0 && p.nrec == 1 && p.a1 == j && p.g0 == 0, "spr %d sub %d rmax %d j %lld j_hi %lld", spr, sub, rmax, j,
                  e);
          }
          for (long long j_hi = j + 1; j_hi <= j + 4LL * spr; j_hi++) {
            long long cur = j;
            while (cur < j_hi) {
              const WelchLaunch p = welch_plan(spr, sub, sb, rmax, cur, j_hi);
              launches++;
              if (!(p.a1 > cur && p.a1 <= j_hi)) { CHECK(false, "a1 %lld outside (%lld, %lld]", p.a1, cur, j_hi); break; }
              long long lo, hi;
              welch_sub(spr, sub, sb, p.g0, lo, hi);
              CHECK(lo <= cur && cur < hi, "g0 %lld does not hold segment %lld", p.g0, cur);
              int runs = 0;
              std::set<long long> recs;
              for (long long g = p.g0;; g++) {
                welch_sub(spr, sub, sb, g, lo, hi);
                if (lo >= p.a1) break;
                const long long c_lo = lo > cur ? lo : cur, c_hi = hi < p.a1 ? hi : p.a1;
                if (c_lo >= c_hi) { CHECK(false, "empty run at sub-block %lld", g); continue; }
                CHECK(c_lo / spr == (c_hi - 1) / spr, "run [%lld, %lld) crosses a record of %d", c_lo, c_hi, spr);
                runs++;
                recs.insert(c_lo / spr);
              }
              CHECK(p.runs == runs && p.nrec == (int)recs.size(), "runs %d (counted %d) nrec %d (counted %zu)", p.runs, runs, p.nrec,
                    recs.size());
              CHECK(p.runs >= 1 && p.runs <= rmax, "runs %d of rmax %d", p.runs, rmax);
              CHECK(p.a1 == j_hi || p.runs == rmax, "a launch of %d < %d runs ends at %lld < %lld", p.runs, rmax, p.a1,
                    j_hi);
              cur = p.a1;
            }
          }
        }
      }
  return launches;
}

// the grid of capacities of the monitors and the analyser, row by row against the fixture
static int check_sizing(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) { printf("FAIL cannot open %s\n", path); fails++; return 0; }
  char line[256];
  auto next = [&]() -> bool {
    while (fgets(line, sizeof line, f)) if (line[0] != '#') return true;
    return false;
  };
  int rows = 0;
  // the monitors (kernels_monitor.hpp): N = 1024, sub-blocks of 4 .. 32, about 512 runs, 1024 at most
  const unsigned ivs[4] = {512u, 512u * 37u, 38400u, 384000u};
  for (int k = 9; k <= 27; k++)
    for (int d = -1; d <= 1; d++)
      for (unsigned interval : ivs) {
        const size_t cap = ((size_t)1 << k) + d;
        const WelchSched w = welch_size(512u, interval, cap, 4, 32, 512, 1024);
        size_t fcap; unsigned fiv; int spr, sub, sb, rmax;
        const bool ok = next() && sscanf(line, "mon %zu %u %d %d %d %d", &fcap, &fiv, &spr, &sub, &sb, &rmax) == 6;
        CHECK(ok && fcap == cap && fiv == interval, "fixture row %d is not mon %zu %u: %s", rows, cap, interval, line);
        CHECK(ok && w.spr == spr && w.sub == sub && w.sb == sb && w.rmax == rmax, "mon %zu %u: %d %d %d %d, recorded %s", cap,
              interval, w.spr, w.sub, w.sb, w.rmax, line);
        CHECK(w.par == 0 && w.n == 0 && w.next_seg == 0 && w.done() == 0, "a fresh cursor");
        rows++;
      }
  // the analyser (kernels_analyser.hpp): sub-blocks of 1 .. 16, about 64 runs, kAnMaxRuns = 128 at most
  for (int k = 9; k <= 27; k++)
    for (int d = -1; d <= 1; d++)
      for (int N = 1024; N <= 8192; N *= 2)
        for (int one = 0; one < 2; one++) {
          const size_t cap = ((size_t)1 << k) + d;
          const unsigned H = (unsigned)N / 2, interval = one ? H : 6u * (unsigned)N;
          const WelchSched w = welch_size(H, interval, cap, 1, 16, 64, 128);
          size_t fcap; unsigned fiv; int fn, spr, sub, sb, rmax;
          const bool ok = next() && sscanf(line, "an %zu %d %u %d %d %d %d", &fcap, &fn, &fiv, &spr, &sub, &sb, &rmax) == 7;
          CHECK(ok && fcap == cap && fn == N && fiv == interval, "fixture row %d is not an %zu %d %u: %s", rows, cap, N, interval,
                line);
          CHECK(ok && w.spr == spr && w.sub == sub && w.sb == sb && w.rmax == rmax, "an %zu %d %u: %d %d %d %d, recorded %s", cap,
                N, interval, w.spr, w.sub, w.sb, w.rmax, line);
          rows++;
        }
  CHECK(!next(), "the fixture has more rows than the grid");
  fclose(f);
  return rows;
}

static bool same(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// welch_tables against the expressions of SegMonitor::init (Hann, N = 1024), AnalyserStage::init (Blackman-Harris) and
// fmr_spectrum::init (spec_window, twiddles as (cos(-t), sin(-t))) as they stood, for every size the stages take
static int check_tables() {
  int tables = 0;
  for (int N = 256; N <= 16384; N *= 2)
    for (int window = 0; window < 3; window++) {
      const WelchTables t = welch_tables(N, window);
      CHECK((int)t.win.size() == N && (int)t.tw.size() == N, "sizes at N %d", N);
      double sw = 0.0, sw2 = 0.0, sumw2_b = 0.0;
      int bad = 0;
      for (int n = 0; n < N; n++) {
        // fmr_spectrum::init
        const double x = 2.0 * M_PI * n / N;
        const double wd = window == 0 ? 0.5 - 0.5 * std::cos(x)
                        : window == 2 ? 0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2 * x) - 0.01168 * std::cos(3 * x)
                                      : 1.0;
        const float w = (float)wd;
        sw += w;
        sw2 += (double)w * w;
        const double a = -2.0 * M_PI * n / N;
        bad += !same(t.win[n], w) || !same(t.tw[n].x, (float)std::cos(a)) || !same(t.tw[n].y, (float)std::sin(a));
        // SegMonitor::init and AnalyserStage::init
        const double tt = 2.0 * M_PI * n / N;
        const float wb = window == 0 ? (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * n / N))
                       : window == 2
                           ? (float)(0.35875 - 0.48829 * std::cos(tt) + 0.14128 * std::cos(2.0 * tt) - 0.01168 * std::cos(3.0 * tt))
                           : 1.f;
        sumw2_b += (double)wb * (double)wb;
        bad += !same(t.win[n], wb) || !same(t.tw[n].x, (float)std::cos(tt)) || !same(t.tw[n].y, (float)-std::sin(tt));
      }
      CHECK(bad == 0, "N %d window %d: %d entries differ from the former expressions", N, window, bad);
      CHECK(same(t.sumw, sw) && same(t.sumw2, sw2) && same(t.sumw2, sumw2_b), "N %d window %d: the sums differ", N, window);
      tables++;
    }
  return tables;
}

int main(int argc, char **argv) {
  if (argc < 2) { printf("usage: welch_plan_check tests/golden/welch_sizing.txt\n"); return 2; }
  const long long launches = check_planner();
  printf("planner %lld launches %s\n", launches, fails ? "FAILED" : "ok");
  int before = fails;
  const int rows = check_sizing(argv[1]);
  printf("sizing %d rows %s\n", rows, fails > before ? "FAILED" : "ok");
  before = fails;
  const int tables = check_tables();
  printf("tables %d %s\n", tables, fails > before ? "FAILED" : "ok");
  return fails ? 1 : 0;
}
