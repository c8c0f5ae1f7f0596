// fmr_detail::Stages (host/fmradion_facade.hpp) on the host, the C functions it calls replaced by stubs that log: what a
// decoder object has enabled is enabled again on a chain made anew, in the order the library wants (monitor, loudness,
// weak signal, IQ correction, blanker, RF monitor, output with its rate, analyser, MPX output), with the configuration it
// was given; what was not enabled, or was refused, is not.  Built under the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#define FMR_FACADE_THROW
#include "../airspy-fmradion_amd/host/fmradion_facade.hpp"

namespace {
struct Call { std::string fn; fmr_chain *chain; std::vector<unsigned char> cfg; };
std::vector<Call> g_log;
std::string g_refuse;      // the function that fails

int logged(const char *fn, fmr_chain *c, const void *cfg, size_t size) {
  if (g_refuse == fn) return FMR_ERR_BAD_ARG;
  const unsigned char *p = static_cast<const unsigned char *>(cfg);
  g_log.push_back({fn, c, std::vector<unsigned char>(p, p + size)});
  return FMR_OK;
}
}  // namespace

extern "C" {
const char *fmr_last_error(void) { return "refused by the stub"; }
int fmr_filter_table(const char *name, const void **data, int *is_double) {      // (FilterParameters' tables, read when the
  static const double taps[3] = {0.0, 0.0, 0.0};                                 // program starts: three zeros of either type)
  *data = taps; *is_double = std::strstr(name, "audio") != nullptr;
  return 3;
}
#define STUB(fn, type) int fn(fmr_chain *c, const type *cfg, size_t size) { return logged(#fn, c, cfg, size); }
STUB(fmr_enable_monitor, fmr_monitor_config)
STUB(fmr_enable_loudness, fmr_loudness_config)
STUB(fmr_enable_weak_signal, fmr_weak_signal_config)
STUB(fmr_enable_iq_correction, fmr_iq_correction_config)
STUB(fmr_enable_blanker, fmr_blanker_config)
STUB(fmr_enable_rf_monitor, fmr_rf_monitor_config)
STUB(fmr_enable_output, fmr_output_config)
STUB(fmr_set_output_rate, fmr_output_rate_config)
STUB(fmr_enable_analyser, fmr_analyser_config)
STUB(fmr_enable_mpx_output, fmr_mpx_output_config)
}

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); g_failed++; } } while (0)

static std::vector<std::string> names() {
  std::vector<std::string> v;
  for (const Call &c : g_log) v.push_back(c.fn);
  return v;
}

int main() {
  fmr_chain *const first = reinterpret_cast<fmr_chain *>(0x1000), *const second = reinterpret_cast<fmr_chain *>(0x2000);
  const std::vector<std::string> all = {"fmr_enable_monitor", "fmr_enable_loudness", "fmr_enable_weak_signal",
                                        "fmr_enable_iq_correction", "fmr_enable_blanker", "fmr_enable_rf_monitor",
                                        "fmr_enable_output", "fmr_set_output_rate", "fmr_enable_analyser", "fmr_enable_mpx_output"};
  {   // nothing enabled: nothing applied
    fmr_detail::Stages s;
    s.apply(second);
    CHECK(g_log.empty());
    CHECK(s.analyser_cfg().max_records == 0 && s.analyser_cfg().fft_size == 0);
  }
  {   // everything, enabled in another order than apply()'s
    fmr_detail::Stages s;
    fmr_blanker_config nb{};
    nb.mode = FMR_NB_ACT; nb.max_records = 15;
    fmr_iq_correction_config iqc{};
    iqc.average_intervals = 8;
    fmr_weak_signal_config ws{};
    ws.highcut_hz = 3000.0;
    s.mpx_output(first, fmr_detail::mpx_output_config(FMR_PCM_F32, 171000, 0.25, 4096));
    s.analyser(first, 2048, 0, 13);
    s.output(first, fmr_detail::output_config(FMR_PCM_F32, 0.0, 0.0, 0, 0), fmr_detail::output_rate_config(32000, true));
    s.rf_monitor(first, 1024, 5);
    s.blanker(first, nb);
    s.iq_correction(first, iqc);
    s.weak_signal(first, ws);
    s.loudness(first, 480, 9);
    s.monitor(first, 1024, 64, 1.5, 7);
    CHECK(g_log.size() == all.size());
    for (const Call &c : g_log) CHECK(c.chain == first);
    const std::vector<Call> enabled = g_log;
    g_log.clear();
    s.apply(second);
    CHECK(names() == all);
    for (const Call &c : g_log) {
      CHECK(c.chain == second);
      bool same = false;     // the configuration the enable passed, struct_size filled in
      for (const Call &e : enabled) same = same || (e.fn == c.fn && e.cfg == c.cfg);
      CHECK(same);
      unsigned size = 0;
      std::memcpy(&size, c.cfg.data(), sizeof size);
      CHECK(size == c.cfg.size());
    }
    CHECK(s.analyser_cfg().max_records == 13 && s.analyser_cfg().fft_size == 2048);
    g_log.clear();
    s.apply(first);          // and again: apply() forgets nothing
    CHECK(names() == all);
    g_log.clear();
  }
  {   // a subset; an output without a rate sets none
    fmr_detail::Stages s;
    s.output(first, fmr_detail::output_config(FMR_PCM_S16, 0.0, 0.0, 0, 0), fmr_detail::output_rate_config(0, false));
    s.blanker(first, fmr_blanker_config{});
    g_log.clear();
    s.apply(second);
    CHECK((names() == std::vector<std::string>{"fmr_enable_blanker", "fmr_enable_output"}));
    g_log.clear();
  }
  {   // a refused enable throws and is not remembered
    fmr_detail::Stages s;
    s.loudness(first, 0, 0);
    g_refuse = "fmr_enable_analyser";
    bool threw = false;
    try { s.analyser(first, 1000, 0, 0); } catch (const std::runtime_error &e) {
      threw = std::string(e.what()) == "fmr_enable_analyser: refused by the stub";
    }
    CHECK(threw);
    g_refuse.clear();
    g_log.clear();
    s.apply(second);
    CHECK((names() == std::vector<std::string>{"fmr_enable_loudness"}));
    // ... and a chain that refuses what the one before it took: apply() throws at that stage
    g_refuse = "fmr_enable_loudness";
    threw = false;
    try { s.apply(second); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
  }
  std::printf(g_failed ? "%d checks failed\n" : "stages ok\n", g_failed);
  return g_failed ? 1 : 0;
}
