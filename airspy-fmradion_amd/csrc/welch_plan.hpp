// welch_plan.hpp -- host side of the Welch segment engine (kernels_welch.hpp): the record partition, a chain's sizing, the
// plan of one launch and the window / twiddle tables.  Pure: no HIP in it, it compiles with the host compiler alone
// (tests/welch_plan_check.cpp); welch_sub is also what the kernels call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#ifdef __HIPCC__
#define FMR_WELCH_HD __host__ __device__
#else
#define FMR_WELCH_HD
#endif

namespace fmr {

// segments [lo, hi) of sub-block g (whole, before a launch clips it): records of spr segments, cut into sb =
// ceil(spr / sub) aligned sub-blocks of `sub` segments, the last one shorter; g = record * sb + sub-block in the record
FMR_WELCH_HD inline void welch_sub(int spr, int sub, int sb, long long g, long long &lo, long long &hi) {
  const long long l = g / sb, b = g - l * sb;
  lo = l * spr + b * sub;
  hi = lo + sub < (l + 1) * spr ? lo + sub : (l + 1) * spr;
}

// A stream's partition and cursor: segments per record / per sub-block, sub-blocks per record, runs per stream and launch;
// which copy of the open records is current; samples seen, segments processed.
struct WelchSched {
  int spr = 0, sub = 0, sb = 0, rmax = 0;
  int par = 0;
  long long n = 0, next_seg = 0;
  unsigned long long done() const { return (unsigned long long)(next_seg / spr); }   // records complete
};

// The partition of a chain whose calls hold at most `cap` samples: a full call in about target_runs runs per stream, with
// sub-blocks of sub_min .. sub_max segments (a run is a workgroup's serial work, and the partition only moves the fp64
// rounding of the sums), and room for max_runs runs per launch at most.
inline WelchSched welch_size(unsigned hop, unsigned interval, size_t cap, int sub_min, int sub_max, int target_runs,
                             int max_runs) {
  WelchSched w;
  w.spr = (int)(interval / hop);
  const size_t max_seg = cap / hop + 2, t = (size_t)target_runs;
  w.sub = (int)std::min<size_t>((size_t)sub_max, std::max<size_t>((size_t)sub_min, (max_seg + t - 1) / t));
  w.sb = (w.spr + w.sub - 1) / w.sub;
  w.rmax = (int)std::min<size_t>((size_t)max_runs, max_seg / w.sub + 2 * (max_seg / w.spr + 2) + 2);
  return w;
}

// The next launch of a call: of the call's segments [j, j_hi) the [j, a1) that fit into rmax runs per stream (run r =
// sub-block g0 + r clipped to them), the runs and the records they touch.  j >= j_hi: no segment is left (runs = 0, and
// one record's blocks for the carry).
struct WelchLaunch {
  long long g0, a1;
  int runs, nrec;
};
inline WelchLaunch welch_plan(int spr, int sub, int sb, int rmax, long long j, long long j_hi) {
  WelchLaunch p{0, j, 0, 1};
  if (j >= j_hi) return p;
  const long long l = j / spr;
  p.g0 = l * sb + (j - l * spr) / sub;
  long long lo, hi;
  welch_sub(spr, sub, sb, p.g0 + rmax - 1, lo, hi);
  p.a1 = std::min(j_hi, hi);
  const long long l_end = (p.a1 - 1) / spr;
  p.runs = (int)(l_end * sb + (p.a1 - 1 - l_end * spr) / sub - p.g0 + 1);
  p.nrec = (int)(l_end - l + 1);
  return p;
}

// The periodic window of kind `window` (the values of FMR_WINDOW_*) and the twiddles tw[i] = exp(-2 pi i i / N), built in
// double and rounded once to fp32, with the sums of the rounded window and of its squares.
enum { kWelchHann = 0, kWelchRect = 1, kWelchBlackmanHarris = 2 };
struct WelchCpx { float x, y; };     // (float2's layout)
struct WelchTables {
  std::vector<float> win;
  std::vector<WelchCpx> tw;
  double sumw = 0.0, sumw2 = 0.0;
};
inline WelchTables welch_tables(int N, int window) {
  WelchTables t;
  t.win.resize((size_t)N);
  t.tw.resize((size_t)N);
  for (int i = 0; i < N; i++) {
    const double x = 2.0 * M_PI * i / N;
    const double w = window == kWelchHann ? 0.5 - 0.5 * std::cos(x)
                   : window == kWelchBlackmanHarris
                       ? 0.35875 - 0.48829 * std::cos(x) + 0.14128 * std::cos(2.0 * x) - 0.01168 * std::cos(3.0 * x)
                       : 1.0;
    t.win[i] = (float)w;
    t.sumw += (double)t.win[i];
    t.sumw2 += (double)t.win[i] * (double)t.win[i];
    t.tw[i] = WelchCpx{(float)std::cos(x), (float)-std::sin(x)};
  }
  return t;
}

}  // namespace fmr
