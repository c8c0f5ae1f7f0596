// fmradion_amd.hip -- host engine + C-ABI (include/fmradion_amd.h) of the
// MI355X-native FM/AM demodulation chain.  One translation unit; the kernels
// are in kernels.hpp.  No CPU fallback: without a HIP device fmr_create fails.
//
// A call processes n_blocks consecutive input blocks of n_streams streams with
// the exact per-block semantics of n_blocks sequential calls of the reference
// classes (block-head FIR path, per-block lock decision, per-block equaliser
// cadence, ... SURVEY.md 8a hazards H1-H5): the time-invariant stages run over
// the whole call at once, the block structure travels as small offset tables
// the host derives from the resampler's integer output-count law.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <array>
#include <atomic>
#include <chrono>
#include <thread>

#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fmradion_amd.h"
#include "design.hpp"
#include "kernels.hpp"
#include "kernels_par.hpp"
#include "kernels_fused.hpp"
#include "kernels_decim16.hpp"
#include "kernels_chanbank.hpp"
#include "kernels_rds.hpp"
#include "welch_plan.hpp"
#include "kernels_spectrum.hpp"
#include "kernels_monitor.hpp"
#include "kernels_loudness.hpp"
#include "kernels_analyser.hpp"
#include "kernels_rfmon.hpp"
#include "kernels_output.hpp"
#include "kernels_mpxout.hpp"
#include "kernels_mpxin.hpp"
#include "kernels_weaksignal.hpp"
#include <complex>
#include "kernels_blanker.hpp"
#include "kernels_iqcorr.hpp"
#include "../host/fmradion_rds.hpp"

namespace {
#include "filter_tables.inc"

thread_local std::string g_err;

void set_err(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return FMR_ERR_HIP;                                                             \
    }                                                                                 \
  } while (0)

constexpr double kFmRate = 384000.0;   // FmDecoder::sample_rate_if   (FmDecode.h:38)
constexpr double kPcmRate = 48000.0;   // FmDecoder::sample_rate_pcm  (FmDecode.h:40)
constexpr double kAmRate = 48000.0;    // AmDecoder::internal_rate_pcm (AmDecode.h:36)
constexpr double kIfAtten = 140.0;     // resampler spec, DESIGN.md (FAST class)
constexpr double kR8bAtten = 180.0, kR8bPassFrac = 0.98;   // R8B class: the defaults of r8b::CDSPResampler24 (IfResampler.cpp:25-29)
constexpr double kAudioAtten = 180.0;
constexpr int FMR_MODE_NONE = -1;
// weak-signal handling: the default thresholds in dB of the smoothed detector reading (DESIGN.md section 16 has the table)
constexpr double kWsBlendLo = -33.0, kWsBlendHi = -23.0, kWsHighcutHi = -15.0, kWsMuteHi = -9.0;
// chunk lengths of the time-parallel recurrences (kernels_par.hpp)
constexpr int C_AGC = 256, C_DC = 64, C_DE = 256, C_AM = 256, C_AM_DE = 128, K_AF_ITERS = 6;
#ifndef FMR_C_PLL_MIN
#define FMR_C_PLL_MIN 32
#endif
constexpr int C_PLL_MIN = FMR_C_PLL_MIN;   // smallest PLL chunk (capacity); the actual length is c_pll
constexpr long long kSmallCall = 8192;   // IF samples: calls up to this size enqueue fewer spare Newton rounds
// ... and cut their blocks into PLL chunks of 16 samples instead of c_pll = 64: a lane integrates its chunk serially whatever
// the call's size, and ONE 65536-sample block (2517 IF samples) is 40 chunks of 64 -- one wave, 52 + 44 us for the two
// passes of a call whose whole budget is ~250 us (main.cpp:916-956 calls block by block) -- or 158 chunks of 16: three
// waves side by side, a quarter of the samples each (round 6)
constexpr int kCPllSmall = 16;
constexpr int kMaxMpfTaps = 1280;         // equaliser taps (4 multipath_stages + 1) the widest form of k_mpf4 holds: 64 lanes x 20
constexpr unsigned kAgcWaitTicks = 50000000u;   // 0.5 s of the 100 MHz clock: how long k_mpf4 waits for a chunk's gains (the AGC
                                                // kernel beside it is three times faster than the equaliser: it never waits in practice)
constexpr int K_AGC_ITERS = 6, K_PLL_ITERS = 4;   // PLL: 2 rounds in lock, 2 spare (an unused round is three launches that return at once: ~6 us measured)

// ---- owners of what the HIP runtime hands out: device memory, page-locked host memory, events, streams.  Each holds one
// resource, is move-only, and gives the resource back (Free) when it dies or takes another; nothing else in this file
// frees.  g_live counts what the owners of the process hold (fmr_debug_live_resources).
std::atomic<long long> g_live{0};
template <class P, auto Free>
struct Owned {
  P p = nullptr;
  Owned() = default;
  Owned(Owned &&o) noexcept : p(o.p) { o.p = nullptr; }
  Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
  ~Owned() { reset(); }
  void reset() { if (p) { (void)Free(p); g_live--; } p = nullptr; }
};

template <class T>
struct DevBuf : Owned<T *, hipFree> {
  size_t n = 0;
  int alloc(size_t count) {      // zeroed; a buffer that holds memory gives it back first
    this->reset();
    n = count ? count : 1;
    HIPCHK(hipMalloc((void **)&this->p, n * sizeof(T)));
    g_live++;
    HIPCHK(hipMemset(this->p, 0, n * sizeof(T)));
    return FMR_OK;
  }
};
static_assert(!std::is_copy_constructible_v<DevBuf<float>> && std::is_move_constructible_v<DevBuf<float>>, "owners are move-only");

template <class T>
struct HostBuf : Owned<T *, hipHostFree> {      // page-locked host memory (not zeroed)
  int alloc(size_t count, unsigned flags) {
    this->reset();
    HIPCHK(hipHostMalloc((void **)&this->p, (count ? count : 1) * sizeof(T), flags));
    g_live++;
    return FMR_OK;
  }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
  int create(unsigned flags = hipEventDefault) {
    reset();
    HIPCHK(hipEventCreateWithFlags(&p, flags));
    g_live++;
    return FMR_OK;
  }
  operator hipEvent_t() const { return p; }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  int create() {      // non-blocking
    reset();
    HIPCHK(hipStreamCreateWithFlags(&p, hipStreamNonBlocking));
    g_live++;
    return FMR_OK;
  }
  operator hipStream_t() const { return p; }
};

struct KernelTime { const char *name; Event a, b; };

// A struct whose first field is struct_size, as the caller of fn knows it (cfg_size bytes, 0 = this library's size) ->
// this library's, zero-filled.  A caller that knows more than the library is refused.
template <class T>
int take_sized(const char *fn, const char *type_name, const T *cfg, size_t cfg_size, T &full) {
  const size_t size = cfg_size ? cfg_size : sizeof(T);
  const size_t stated = size >= sizeof(unsigned) ? (size_t)cfg->struct_size : (size_t)0;
  if (size > sizeof(T) || stated > sizeof(T)) {
    set_err("%s: struct_size %zu is larger than this library's %s (%zu): the caller is newer than the library", fn,
            std::max(size, stated), type_name, sizeof(T));
    return FMR_ERR_BAD_ARG;
  }
  memset(&full, 0, sizeof full);
  memcpy(&full, cfg, size);
  return FMR_OK;
}
// ... and the way back: at most the caller's out_size bytes (0 = this library's size) of full
template <class T>
void give_sized(void *out, size_t out_size, const T &full) {
  const size_t size = out_size ? out_size : sizeof full;
  memcpy(out, &full, size < sizeof full ? size : sizeof full);
}

}  // namespace

using namespace fmr;

namespace {
// The reader's side of a ring of L records per stream (the three monitors' records, the waterfall's lines): per stream
// the next unread record and the records overwritten unread.  `done` is the number of records complete so far.
struct RecCursor {
  std::vector<unsigned long long> read, dropped;
  unsigned long long L = 1;
  void reset(int streams, int depth) { read.assign(streams, 0); dropped.assign(streams, 0); L = (unsigned long long)depth; }
  // records the ring has overwritten unread: the read position follows, the loss is counted
  void catch_up(int s, unsigned long long done) {
    if (done > L && read[s] < done - L) {
      dropped[s] += done - L - read[s];
      read[s] = done - L;
    }
  }
  // Drains up to cap records of stream s, oldest first: copy(k, slot, m) fetches records k .. k + m of the read from the
  // ring slots slot .. slot + m and returns FMR_OK, or an error that ends the read with nothing drained.  Returns the
  // count; cap = 0 returns the number waiting and drains nothing.
  template <class F>
  int take(int s, unsigned long long done, unsigned long long cap, F &&copy) {
    catch_up(s, done);
    const unsigned long long first = read[s], ready = std::min<unsigned long long>(done - first, (unsigned long long)INT_MAX);
    const size_t n = (size_t)std::min(ready, cap);
    for (size_t k = 0; k < n;) {       // the ring slots first % L .. in at most two contiguous pieces
      const size_t slot = (size_t)((first + k) % L), m = std::min(n - k, (size_t)L - slot);
      if (int rc = copy(k, slot, m)) return rc;
      k += m;
    }
    read[s] = first + n;
    return (int)(cap == 0 ? ready : n);
  }
};

// The engine of the modulation monitor and the RF monitor (kernels_monitor.hpp): records of `interval` samples cut into
// aligned sub-blocks of segments, the window and twiddle tables, the stream's carry, the runs' partials, the open records
// (two copies by launch parity) and the rings of max_records records per stream with their reader.  It counts in absolute
// samples (n), so the cut into calls does not matter.  fmr_chain::seg_stage runs a call through it.
// The modulation monitor (fmr_enable_monitor) is a second reader of the call's MPX at the head of the
// audio tail, beside the RDS stage; the RF monitor (fmr_enable_rf_monitor; kernels_rfmon.hpp) is a
// second instance that reads the call's IF ring slot (the decoder's input, or |x|^2 behind a discriminator epilogue).
// This and the four stages below are the OPTIONAL stages of a chain: each owns all its state (build_stage).
struct SegMonitor {
  bool on = false;
  unsigned interval = 0;                     // samples per record
  int bins = 0;                              // histogram counters per record
  double hist_range = 0.0;                   // modulation monitor: the histogram covers +- this (the RF monitor's bin rule takes none)
  WelchSched ws;                             // the partition, the open records' parity, samples seen, segments processed
  double sumw2 = 0.0;
  DevBuf<float> d_win, d_carry;
  DevBuf<float2> d_tw;
  DevBuf<double> d_ppsd, d_open_psd, d_ring_psd;
  DevBuf<unsigned> d_phist, d_open_hist, d_ring_hist;
  DevBuf<MonRec> d_prec, d_open_rec, d_ring_rec;
  RecCursor cur;
  unsigned long long done() const { return ws.done(); }
  int init(int S, size_t max_if, unsigned interval_samples, int hist_bins, double range, int max_records);
};
// both monitors' kernels (k_mon_seg<Src>, k_mon_reduce<Src>) as seg_stage takes them
using MonSegFn = decltype(&k_mon_seg<MonMpxSrc>);
using MonReduceFn = decltype(&k_mon_reduce<MonMpxSrc>);

// RDS (fmr_create_rds; kernels_rds.hpp, host/fmradion_rds.hpp).  The stage runs at the head of the
// audio tail (fmr_chain::rds_stage): it reads the call's MPX from the base slot and carries everything else in buffers of
// its own (MPX history, y1 / y2 rings, RdsState), which only it writes.  The bits of a call go to a slot of a ring of
// page-locked host slots; k_signal_host marks the slot filled and the host decoders drain it (drain).
struct RdsStage {
  bool on = false;
  static constexpr int kSlots = 8;
  int S = 0;
  int R = 0, maxw = 0;                       // ring length (power of two), windows per call
  size_t slot_stride = 0;                    // bytes per stream in a host slot
  DevBuf<float> d_h1, d_h2, d_xhalo;
  DevBuf<float2> d_lo, d_y1, d_y2;
  DevBuf<RdsState> d_state;
  DevBuf<RdsEst> d_est;
  DevBuf<RdsRec> d_rec;
  HostBuf<char> h_slots;
  HostBuf<unsigned long long> h_mark;        // calls whose RDS slot is filled
  long long n = 0, w = 0;                    // MPX samples seen, next window
  unsigned long long seq = 0, drained = 0;
  unsigned long long tap_seq = 0;            // slot of the most recent call's windows (0: it completed none): fmr_debug_read 5
  double gain = 1.0;                         // |soft symbol| of a unit subcarrier (injection estimate)
  std::vector<fmr_rds::Decoder> dec;
  std::vector<RdsSlotHdr> hdr;
  int init(int streams, size_t max_if);
  void drain();
};

// Audio monitor (fmr_enable_loudness; kernels_loudness.hpp).  A reader of the call's finished audio
// behind the output mux, on the tail's stream (fmr_chain::ld_stage): it counts in absolute audio samples (n) and keeps its
// own carries (the K-weighting state, the true-peak history, the open record).
struct LoudnessStage {
  bool on = false;
  fmr_loudness_config cfg{};                 // the defaults filled in
  int cps = 0, rmax = 0, par = 0;            // chunks per sub-block, runs per stream and launch, current copy of the open records
  long long n = 0;                           // audio samples seen (per channel)
  LdCoef coef{};
  DevBuf<double> d_pw, d_taps, d_G, d_start, d_pkw, d_state, d_hist;
  DevBuf<LdPart> d_part;
  DevBuf<LdRec> d_open, d_ring;
  RecCursor cur;
  unsigned long long done() const { return (unsigned long long)(n / (long long)cfg.step_samples); }   // records complete
  int init(int S, size_t max_au, const fmr_loudness_config &m);
};

// Audio analyser (fmr_enable_analyser; kernels_analyser.hpp).  A second reader of the call's finished
// audio behind the output mux, on the stream that wrote it (fmr_chain::an_stage), in every decoder mode: it counts in
// absolute audio frames (n) and keeps its own carry (the last N frames), partials, open records and rings.
using AnSegFn = decltype(&k_an_seg<kAnLogMin>);
struct AnalyserStage {
  bool on = false;
  fmr_analyser_config cfg{};                 // the defaults filled in
  int N = 0, H = 0, nb = 0, logn = 0;        // fft_size, hop, bins per row = N / 2 + 1
  WelchSched ws;                             // the partition, the open records' parity, frames seen, segments processed
  int threads = 0, lds = 0;                  // of k_an_seg at this N
  AnSegFn kseg = nullptr;
  double sumw2 = 0.0;
  DevBuf<float> d_win;
  DevBuf<float2> d_tw;
  DevBuf<double> d_carry, d_ppsd, d_open_psd, d_ring_psd;
  DevBuf<AnPart> d_ppart;
  DevBuf<AnRec> d_open_rec, d_ring_rec;
  RecCursor cur;
  unsigned long long done() const { return ws.done(); }
  int init(int S, size_t max_au, const fmr_analyser_config &m);
};

// Rate converter of the output stage (fmr_set_output_rate): with `on` the ring is written by
// k_out_rate from the staged z instead of by k_out_pcm, oframes counts its frames, and the stream's clip / non-finite
// totals live in d_tot.  Two staging rows: a call's z goes behind the T - 1 frames of history at the head of row zpar,
// and what it leaves as history to the head of the other row.
struct OutRate {
  bool on = false, mono = false;
  int hz = kOutRateIn;
  OutRateGeom geom{1, 1, 1, 0, 0, 0};
  unsigned long long oframes = 0;
  int zpar = 0;
  DevBuf<double> d_z, d_taps;                // [2][S][zstride]; the prototype, T L
  DevBuf<unsigned long long> d_tot;          // [S][2]
  int init(int rate, bool to_mono, int S, bool stereo, size_t max_au);
};

// Output stage (fmr_enable_output; kernels_output.hpp).  The last reader of the call's finished
// audio, on the stream that wrote it (fmr_chain::out_stage): squelch, gain and PCM conversion into a ring of frames per
// stream, and one record per block with the stream loop's meters.  The block, frame and record counters live here and are
// taken when a call is issued (begin); the device carries the two levels.  k_stats leaves every block's IF RMS in the
// call's slot of d_ifrms (the tail of a pipelined chain runs a call late).
struct OutputStage {
  bool on = false;
  bool stereo = false;                       // of the chain
  fmr_output_config cfg{};                   // the defaults filled in
  unsigned long long block = 0, recs = 0, frames = 0;   // blocks handed in, records and audio frames produced
  size_t ifrms_slot_len = 0;                 // S max_blocks of the chain
  DevBuf<float> d_ifrms;                     // [slots][S][max_blocks]
  DevBuf<OutPart> d_part;                    // [S][max_blocks]
  DevBuf<float2> d_state;                    // [S] if_level, audio_level
  DevBuf<OutRec> d_rec;                      // [S][max_blocks of the config]
  DevBuf<unsigned char> d_pcm;               // [S][max_frames] frames
  RecCursor fcur, bcur;                      // frames, records
  bool rate_set = false;                     // fmr_set_output_rate has been called (48000 stereo leaves `rate` as it is)
  OutRate rate;
  int channels() const { return stereo && !(rate.on && rate.mono) ? 2 : 1; }     // of the ring
  unsigned long long produced() const { return rate.on ? rate.oframes : frames; }   // ring frames
  size_t frame_bytes() const { return (size_t)channels() * (cfg.format == FMR_PCM_F32 ? 4 : 2); }
  float *ifrms_slot(int q) { return on ? d_ifrms.p + (size_t)q * ifrms_slot_len : nullptr; }
  int init(int S, bool chain_stereo, int max_blocks, int slots, const fmr_output_config &m);
  OutArgs begin(unsigned long long block0, const int *if_len, int nb, long long N_au);
};

// MPX output (fmr_enable_mpx_output; kernels_mpxout.hpp).  One more reader of the call's MPX at the head
// of the audio tail (fmr_chain::mpxout_stage): the composite at rate = 384000 L / M as PCM into a ring of mono frames per
// stream.  The sample and frame counters and the carry's parity live here and are taken when a call is issued (begin): the
// pipelined tail runs a call late.  The device carries the last T - 1 MPX samples (two rows by call parity, written by the
// stage on the tail's stream) and the stream's clip / non-finite totals.
struct MpxOutStage {
  bool on = false;
  fmr_mpx_output_config cfg{};               // the defaults filled in
  MpxOutGeom geom{1, 1, 1, 0};
  unsigned long long n = 0, oframes = 0;     // MPX samples handed in, ring frames produced: ceil(n L / M)
  int par = 0;
  DevBuf<double> d_taps;                     // the prototype, T L (none at 384000)
  DevBuf<float> d_carry;                     // [2][S][T - 1] (none at 384000)
  DevBuf<unsigned long long> d_tot;          // [S][2]
  DevBuf<unsigned char> d_pcm;               // [S][max_frames] samples
  RecCursor cur;
  size_t frame_bytes() const { return cfg.format == FMR_PCM_F32 ? 4 : 2; }
  int init(int S, const fmr_mpx_output_config &m);
  MpxOutArgs begin(long long N_if);
};

// MPX input (fmr_create_mpx_decoder; kernels_mpxin.hpp).  The front end of a chain that is fed PCM: it
// stands where IF resampler, IF AGC and discriminator stand on an IQ chain (fmr_chain::mpxin_stage, on the decoder stream) and
// writes the call's MPX row, its float copy and the per-block baseband sums.  The frame and sample counters and the
// carry's parity live here; plan_call reads them for the count law, mpxin_stage advances them (begin).  The device carries
// the last K - 1 frames as u (two rows by call parity) and the streams' non-finite totals; d_pcm takes the rows of the
// host entry point (fmr_process_mpx_blocks).  Built by init() of such a chain and of no other.
struct MpxInStage {
  bool on = false;
  MpxInGeom geom{1, 1, 1, 1, 0};
  int format = FMR_PCM_S16;
  double gain = 1.0, g = 1.0;                // as configured; gain M / L (the kernels' factor)
  unsigned long long frames = 0, samples = 0;   // frames taken, MPX samples made of them: ceil(frames M / L)
  int par = 0;
  DevBuf<double> d_taps;                     // the prototype padded to K M (none at 384000)
  DevBuf<double> d_carry;                    // [2][S][K - 1] (none at 384000)
  DevBuf<double> d_s16;                      // FMR_PCM_S16: v / 32767.0 for every v, formed here on the host ([v + 32768])
  DevBuf<unsigned long long> d_tot;          // [S]
  DevBuf<unsigned char> d_pcm;               // [S][max_in] frames
  size_t frame_bytes() const { return format == FMR_PCM_F32 ? 4 : 2; }
  unsigned long long samples_after(unsigned long long f) const {      // the count law
    return (f * (unsigned long long)geom.M + (unsigned long long)geom.L - 1) / (unsigned long long)geom.L;
  }
  int init(int S, size_t max_in, int rate, int fmt, double gain_);
  MpxInArgs begin(long long n_frames);
};

// Weak-signal handling (fmr_enable_weak_signal; kernels_weaksignal.hpp).  Two halves on the tail's
// stream: the detector and the control read the call's MPX beside the other MPX readers (fmr_chain::ws_measure); in
// FMR_WS_ACT the action rewrites the finished audio directly behind the output mux (fmr_chain::ws_act).  The sample and
// frame counters live here and are taken when a call is issued (begin): the pipelined tail runs a call late.  The device
// carries s, the open interval and record, the MPX history and the high cut's state.
struct WsArgs { long long n0 = 0, n1 = 0, f0 = 0, f1 = 0; };     // the call's MPX samples [n0, n1) and audio frames [f0, f1)
struct WeakSignalStage {
  bool on = false;
  fmr_weak_signal_config cfg{};              // the defaults filled in
  WsCoef coef{};
  double alpha = 0.0, drop = 0.0;            // the high cut's coefficient, 1 - g_floor
  int pmax = 0, cring = 0, rmax = 0;         // interval pieces and audio chunks of a call at most, control ring length (2^k)
  long long n = 0, f = 0;                    // MPX samples and audio frames handed in
  DevBuf<double> d_h, d_pw, d_G, d_start;
  DevBuf<float> d_hist;
  DevBuf<WsPart> d_part;
  DevBuf<WsState> d_state;
  DevBuf<WsCtl> d_ctl;
  DevBuf<WsRec> d_ring;
  RecCursor cur;
  unsigned long long intervals() const { return (unsigned long long)(n / kWsQ); }
  unsigned long long done() const { return intervals() / (unsigned long long)cfg.record_intervals; }   // records complete
  int init(int S, size_t max_if, size_t max_au, const fmr_weak_signal_config &m);
  WsArgs begin(long long N_if, long long N_au) {
    WsArgs a{n, n + N_if, f, f + N_au};
    n += N_if; f += N_au;
    return a;
  }
};

// What the two stages on the capture share (the impulse blanker and the IQ corrector below; DESIGN.md sections 17 and 18).
// Such a stage runs at the head of a call on the decoder stream, where CallCtx receives the input, its records kernel on
// the side stream behind an event of the stage's own.  It counts in absolute input samples per row (n), cut into intervals
// of kNbQ.  When it acts, the call's readers get its rows instead of the caller's: two row buffers by call parity, because
// a reader of call N's rows (the input history, on the side stream of an in_order chain) may still be pending when call
// N + 1 is written; it is done before call N + 1's front end, which the stage's call N + 2 follows on the same stream.
// The parts of a call are kept twice as well (by the stage: their type is its own): the records kernel of call N reads
// them beside call N + 1, and call N + 2 waits for that kernel's event (ev_rec) before it writes them again.
// A call is begin(), the stage's kernels with out_rows() where it writes rows, and finish().
struct CaptureStage {
  bool on = false, act = false;              // act: the stage rewrites the rows (FMR_NB_ACT / FMR_IQC_ACT)
  int rows = 0, pmax = 0;                    // input rows, pieces of a call at most
  int record_intervals = 1;
  size_t pitch = 0;                          // samples between the rows of a row buffer (one more under an odd caller's stride)
  long long n = 0;                           // samples handed in per row
  unsigned long long calls = 0;              // calls that brought samples
  const float2 *last_rows = nullptr; long long last_stride = 0, last_n = 0;    // acting: the rows the last call wrote
  DevBuf<float2> d_rows[2];
  Event ev_rec[2];
  RecCursor cur;
  // one call: its samples [n0, n1) of every row, the intervals they touch, the parity of its parts and rows, the rows it writes
  struct Call { long long n0 = 0, n1 = 0; int pieces = 0, par = 0; float2 *out = nullptr; long long ostride = 0; };
  unsigned long long intervals() const { return (unsigned long long)(n / kNbQ); }
  unsigned long long done() const { return intervals() / (unsigned long long)record_intervals; }   // records complete
  int init(int rows_, size_t max_in, bool act_, int record_intervals_, int max_records);
  int begin(Call &k, const char *noun, long long N_in, hipStream_t stream);
  void out_rows(Call &k, const float2 *d_iq, size_t stride) const;
  int finish(const Call &k, hipStream_t side, const float2 *&d_iq, size_t &stride);
};

// Impulse blanker on the capture (fmr_enable_blanker; kernels_blanker.hpp), fmr_chain::nb_stage: the
// level and the apply kernel in front of the front end, the records on the side stream behind ev_apply.
struct BlankerStage : CaptureStage {
  fmr_blanker_config cfg{};                  // the defaults filled in
  NbCoef coef{};
  int aring = 0;                             // ring of A per row (2^k)
  DevBuf<NbPart> d_part;                     // [2][rows][pmax]
  DevBuf<unsigned long long> d_aring;        // [rows][aring]
  DevBuf<unsigned char> d_carry;             // [2][rows][G + M]
  DevBuf<NbState> d_state;
  DevBuf<NbRec> d_ring;
  Event ev_apply;
  int init(int rows_, size_t max_in, const fmr_blanker_config &m);
};

// DC-offset and IQ-imbalance correction on the capture (fmr_enable_iq_correction; kernels_iqcorr.hpp),
// in front of the blanker (fmr_chain::iqc_stage): moments, coefficients and, in FMR_IQC_ACT, the apply kernel on the decoder
// stream, the records on the side stream behind ev_coef.
struct IqCorrectionStage : CaptureStage {
  fmr_iq_correction_config cfg{};            // the defaults filled in
  IqcCoef coef{};
  int tring = 0;                             // ring of running totals per row (2^k)
  int tiles() const { return (pmax + kIqcCoefT - 1) / kIqcCoefT; }
  DevBuf<IqcPart> d_part;                    // [2][rows][pmax]
  DevBuf<IqcSum> d_tot;                      // [rows][tiles][(kIqcBack + 1) kIqcCoefT + 1]: the running totals a k_iqc_coef workgroup forms
  DevBuf<IqcSum> d_tring;                    // [rows][tring]
  DevBuf<IqcState> d_state;
  DevBuf<IqcRec> d_ring;
  Event ev_coef;
  int init(int rows_, size_t max_in, const fmr_iq_correction_config &m);
};

}  // namespace

// Diagnostic switches from the environment, read ONCE when a chain is created (INTEGRATION.md section 4 lists them);
// nothing on the call path touches the environment.
struct EnvKnobs {
  // Run-time switches (environment).  Everything else that rounds 1 and 2 compared side by side has been decided and
  // removed; what is left selects a MODE of the product or the slower form a test compares the product with.
  bool serial = false;          // FMR_SERIAL=1       serial recurrence kernels (reference loop order on one lane)
  int pipeline = -1;            // FMR_PIPELINE=0/1   the three stages of a call (front end | PLL | audio tail) of consecutive calls
                                //                    beside each other (1, the default for FM chains with the resampler) or one
                                //                    in-order chain per call (0: the form the tests compare the product with)
#ifdef FMR_AB_PARTNERS
  int test_agc_late = 0;        // FMR_TEST_AGC_LATE=ms test hook (equaliser chain): the AGC kernel beside the equaliser starts this late; -1: never
#endif
  int fe_cus = 0;               // FMR_FE_CUS=n       pipelined chain: workgroups (= CUs) the persistent front-end kernel takes
                                //                    (0: all but one per XCD)
  bool debug_taps = false;      // FMR_DEBUG_TAPS=1   keep intermediate signals readable through fmr_debug_read
  bool host_prof = false;       // FMR_HOST_PROF=1    host enqueue time per call on stderr
  bool no_fused = false;        // FMR_NO_FUSED=1     three-kernel front end, 384 k -> 48 k stage B on the vector ALUs (tests: the product against the form it replaced)
  bool x_pll_chain_head = false; // FMR_X_PLL_CHAIN_HEAD=1  the PLL's second pass runs its down-sweep as two chains of 32 steps, not as a descent
                                //                    through the Jacobian pass's tree (tests and A/B runs: the product against the form it replaced)
#ifdef FMR_AB_PARTNERS          // (libfmradion_amd_ab.so only: the slower forms two GPU tests compare the product with, and a test hook)
  bool pll_v1 = false;          // FMR_PLL_V1         seven launches per Newton round of the PLL instead of three: no hand-off
                                //                    between workgroups inside a launch (tests: bit-equality stress test)
#else
  static constexpr bool pll_v1 = false;
  static constexpr int test_agc_late = 0;
#endif
  double pll_rtol = -1.0;       // FMR_PLL_RTOL       PLL acceptance threshold (< 0 = default)
  bool fe_stamps = false;       // FMR_FE_STAMPS=1    diagnostics: every front-end workgroup leaves its start / end time and hardware id (fmr_debug_read 5)
  bool evt_markers = false;     // FMR_EVT_MARKERS=1  diagnostics: time the fused front end between two event MARKERS on its stream (rounds 1-5) instead of
                                //                    with the start / stop events of its own dispatch
#ifdef FMR_DIAG_KNOBS           // (diagnostic builds under tools/ only: what an A/B run varies without a rebuild)
  int x_spare_aside = -1;       // FMR_X_SPARE_ASIDE=n  the PLL's spare rounds go to the side stream for calls of <= n blocks
  int x_cpll = 0;               // FMR_X_CPLL=n         PLL chunk length
  int x_ballast = 0;            // FMR_X_BALLAST=mask   8 KB of LDS ballast (keeps a kernel off the front end's compute units): 1 lock walk, 2 commit
  int x_amtol = 0;              // FMR_X_AMTOL=n        AM: the IF AGC's acceptance from round 3 on, in 1e-6 (0: the product's 5e-6; 1000 + n: from round 2 on)
  int x_sumw = -1;              // FMR_X_SUMW=n         weight of a macro tile with partial sums, in 1/1000 above 1 (default kFusedSumWeight)
#else
  static constexpr int x_spare_aside = -1, x_cpll = 0, x_ballast = 0, x_sumw = -1, x_amtol = 0;
#endif
  static bool on(const char *n) { const char *e = getenv(n); return e && e[0] == '1'; }
  static bool set(const char *n) { return getenv(n) != nullptr; }
  void load() {
    serial = on("FMR_SERIAL"); debug_taps = on("FMR_DEBUG_TAPS");
    auto num = [](const char *n, int dflt) { const char *e = getenv(n); return (e && e[0]) ? atoi(e) : dflt; };
    pipeline = num("FMR_PIPELINE", -1); fe_cus = num("FMR_FE_CUS", 0);
    host_prof = on("FMR_HOST_PROF"); no_fused = on("FMR_NO_FUSED"); x_pll_chain_head = on("FMR_X_PLL_CHAIN_HEAD");
    fe_stamps = on("FMR_FE_STAMPS"); evt_markers = on("FMR_EVT_MARKERS");
#ifdef FMR_AB_PARTNERS
    test_agc_late = num("FMR_TEST_AGC_LATE", 0); pll_v1 = set("FMR_PLL_V1");
#endif
    if (const char *e = getenv("FMR_PLL_RTOL")) if (e[0]) pll_rtol = atof(e);
#ifdef FMR_DIAG_KNOBS
    x_spare_aside = num("FMR_X_SPARE_ASIDE", -1); x_cpll = num("FMR_X_CPLL", 0); x_ballast = num("FMR_X_BALLAST", 0); x_sumw = num("FMR_X_SUMW", -1); x_amtol = num("FMR_X_AMTOL", 0);
#endif
  }
};

// k_ifr_decim2, 128 lanes per workgroup (256 -- half the tile-halo over-fetch, twice the LDS per workgroup -- measured no
// faster in round 2): kDecim2Out outputs per tile, and the padded row length of its LDS tile for qa taps per phase
constexpr int kDecim2Lanes = 128, kDecim2Out = 2 * kDecim2Lanes;
static int decim2_pad(int qa) {
  int s_pad = kDecim2Out + qa;
  while ((s_pad & 15) != 2) s_pad++;
  return s_pad;
}

#include "chain_shape.hpp"

// The chain: its shape (what plan_create() decided; the call path reads those members as its own), and what init() built
// from it -- streams, events, tables, buffers -- plus the state calls carry.
struct fmr_chain : ChainShape {
  EnvKnobs env;
  Stream stream;
  // side stream: per-block bookkeeping (statistics EMAs, PLL lock logic / PPS) runs beside the
  // audio chain instead of in front of it
  bool dec_valid = true;
  bool if_valid = true;                 // the IF samples of the last call are in last_if (false: the fused front end's discriminator epilogue kept them on chip and stored |x|^2 there)
  bool gain_valid = true;               // the per-sample AGC gains of the last call are in d_gain (fmr_debug_read 4)
  DevBuf<double> d_de_pow;
  DevBuf<double> d_pll_wgr, d_pll_pre, d_pll_te;
  DevBuf<PllSync> d_pll_sync;
  DevBuf<unsigned int> d_pll_tick2;
  int pll_jac_rounds = 1;                // rounds that re-integrate the sensitivities
  double hp_fe = 0, hp_tab = 0, hp_dec = 0; long long hp_calls = 0;   // FMR_HOST_PROF=1
  // ---- cross-call pipelining (FM chains with the resampler; DESIGN.md section 5 "Three stages in flight").  A call is
  // three stages on three streams -- front end (fe: IfResampler + discriminator), PLL stage (stream / side / side2:
  // statistics, AGC, pilot PLL, lock logic) and audio tail (tail: de-emphasis, audio resampler, pilot cut, DC block,
  // mux) -- and stage k of call N runs beside stage k-1 of call N+1.  What one stage hands the next lives in a ring
  // of kPipe slots (IF samples, MPX, L-R, partial sums, per-block lock flags); a slot is refilled once the tail of the
  // call that used it kPipe calls ago has finished (h_marks.p[1], polled by the host).  Everything a stage carries from
  // call to call (halos, StreamState fields) is written by that stage only.
  Stream tail;
  static constexpr int kPipe = 4;        // ring slots
  unsigned long long pipe_seq = 0;       // decoded calls issued (slot = pipe_seq % kPipe)
  int ring_prev = -1;                    // slot of the previous decoded call (-1: none yet) and its IF sample count:
  long long ring_prev_n = 0;             //   the halos of the next slot are carried over from there
  DevBuf<float2> d_if_pp[kPipe];         // slots 1 .. kPipe-1 (slot 0 = d_if / d_base / d_raw / d_fused_part / d_stereo_blk)
  DevBuf<double> d_base_pp[kPipe], d_raw_pp[kPipe];
  DevBuf<FusedPart> d_part_pp[kPipe];
  DevBuf<int> d_stereo_pp[kPipe];
  float2 *if_slot(int q) { return q ? d_if_pp[q].p : d_if.p; }
  fm_mpx_t *base_slot(int q) { return reinterpret_cast<fm_mpx_t *>(q ? d_base_pp[q].p : d_base.p); }   // FM: the MPX as floats (the allocation is shared with the 48 kHz modes' double signal)
  double *raw_slot(int q) { return q ? d_raw_pp[q].p : d_raw.p; }
  FusedPart *part_slot(int q) { return q ? d_part_pp[q].p : d_fused_part.p; }
  int *stereo_slot(int q) { return q ? d_stereo_pp[q].p : d_stereo_blk.p; }
  float2 *last_if = nullptr;
  Event ev_fe[kPipe];
  bool disc_commit_on_side = false;      // the last decoded call's discriminator phase is committed by its k_stats (side stream)
  int sync_all() {                       // every stream of the chain is idle afterwards
    if (int rc = flush_tail(nullptr)) return rc;
    for (hipStream_t st : {stream.p, side.p, side2, tail.p})
      if (st) HIPCHK(hipStreamSynchronize(st));
    return FMR_OK;
  }
  Stream side, side2_own;
  hipStream_t side2 = nullptr;       // the IF AGC when it is off the critical path: side2_own, or on a pipelined chain the side stream
  Event ev_pll1;                     // pipelined chain: the PLL's second pass is done (the passes after it may run on the side stream)
  Event ev_disc, ev_pll, ev_stats, ev_fin, ev_if, ev_agc, ev_tab, ev_mono;
  bool ev_agc_live = false;            // ev_agc has been recorded by an earlier call
  // counters
  ResamplerCounter rsc, arsc;
  unsigned long long abs_in = 0;          // absolute input sample index (FourthConverter phase)
  unsigned wait_multipath_blocks = 100;   // FmDecode.cpp:33
  // device buffers
  DevBuf<float2> d_in, d_in_halo, d_mid, d_if, d_fir, d_mpf, d_mpf_coeff, d_mpf_state;
  // FM with the equaliser: the serial IF AGC runs beside the equaliser kernel, which follows its progress counter
  // (IF samples of this call whose gain is in HBM, per stream; zeroed at the head of every call)
  DevBuf<unsigned long long> d_agc_progress;
  std::vector<unsigned> agc_timeouts_seen;      // per stream: StreamState::agc_sync_timeouts already reported
  bool agc_beside_mpf = false;
  DevBuf<int> d_bphi, d_boff;          // stage-B per-position tap phase / sample offset (k_ifr_poly2)
  DevBuf<float2> d_ft_pre, d_ft_post;   // FineTuner tables (480 entries), empty = no mixer at that place
  unsigned ft_index = 0;                 // FineTuner::m_index, the same for every tuner of the chain
  DevBuf<float> d_afrag_fir_fm;
  DevBuf<float> d_afrag_fir;
  DevBuf<_Float16> d_afrag5h;
  DevBuf<float> d_afrag;               // v4: constant A fragments
  // fused front end (kernels_fused.hpp): stage A + stage B + discriminator in one persistent kernel
  DevBuf<unsigned short> d_dec16_afrag;
  DevBuf<float> d_run_ph;              // R8B / FM -f epilogues [S][workgroup][2]: phases on either side of the workgroups' run boundaries (k_poly5h_heads)
  DevBuf<float> d_hB_last;             // stage-B tap row of position 47
  DevBuf<unsigned short> d_fused_afragA;   // stage-A tap fragments (fp16 high / low terms, both parities)
  DevBuf<unsigned short> d_fused_afragB;   // stage-B tap fragments (fp16 high / low terms) and the inverse of their scale
  float fused_hB_inv_scale = 1.f;
  DevBuf<FusedPart> d_fused_part;
  DevBuf<float> d_fused_mid32;              // per front-end workgroup: fp32 copies of mid samples beyond fp16's range (FusedRing::at32)
  DevBuf<float> d_zero16;                   // sixteen zero bytes (fused front end: the loader's source beyond the ends of a call)
  DevBuf<unsigned long long> d_fe_stamps;   // FMR_FE_STAMPS=1: {start, end, hardware id} of every workgroup of the last fused launch
  int fe_stamps_n = 0;                      //   ... and how many workgroups that launch had
  // The dominant kernel is timed with the start / stop events of ITS OWN dispatch (hipExtLaunchKernelGGL): the time stamps
  // the command processor takes when the kernel's first wave starts and its last wave has ended -- what rocprofv3's kernel
  // trace reads -- and no marker packets on the decoder stream (two markers around a kernel cost 7-10 us of the step and
  // put their own processing time, ~4 us, into the interval).  Set by timed_on for the launch it wraps.
  hipEvent_t ext_a = nullptr, ext_b = nullptr;
  int n_cu = 256;                      // compute units of the device (read at create)
  DevBuf<float> d_hBp;                 // zero-padded tap rows for v3
  DevBuf<float> d_hpA;                 // stage-A taps in polyphase order [D][Q] (k_ifr_decim2)
  unsigned fe_forms_a = 0, fe_forms_b = 0;   // FMR_FE_* bits of the stage-A / stage-B forms launched since create
  // channel bank: stage A in k_ifr_chan (kernels_chanbank.hpp)
  DevBuf<float2> d_cb_taps;                // modulated stage-A taps [group][k][FMR_CB_G]
  DevBuf<ChanPhase> d_cb_ph;                // per channel: f mod F, f D mod F
  unsigned cb_forms = 0;                    // FMR_CB_* bits launched since create
  // ---- optional stages (the structs above say what each is).  Nothing of a stage exists on a chain that never enabled it.
  RdsStage rds;
  SegMonitor mon, rfm;
  LoudnessStage ld;
  AnalyserStage an;
  OutputStage out;
  WeakSignalStage ws;
  MpxOutStage mpxo;
  MpxInStage mpxi;
  BlankerStage nb;
  IqCorrectionStage iqc;
  int iqc_stage(const float2 *&d_iq, size_t &stride, long long N_in);
  int nb_stage(const float2 *&d_iq, size_t &stride, long long N_in);
  int ws_measure(const fm_mpx_t *base, const WsArgs &a, hipStream_t st);
  int ws_act(double *d_aud, long long astride, const WsArgs &a, hipStream_t st);
  int rds_stage(const fm_mpx_t *base, long long N, hipStream_t st);
  int mpxout_stage(const fm_mpx_t *base, const MpxOutArgs &a, hipStream_t st);
  // one call's N samples per stream through monitor m on stream st: the source as kseg / kreduce read it (from, stride, off)
  int seg_stage(SegMonitor &m, const void *from, long long stride, int off, float rf, float scale, MonSegFn kseg,
                MonReduceFn kreduce, const char *seg_name, const char *reduce_name, long long N, hipStream_t st);
  int ld_stage(const double *d_aud, long long astride, long long N, hipStream_t st);
  int an_stage(const double *d_aud, long long astride, long long N, hipStream_t st);
  int out_stage(const double *d_aud, long long astride, const BlockTab &bt, const float *if_rms_blk, const OutArgs &a, hipStream_t st);
  // front end only (fmr_resample_blocks_device): stage B writes row s of this call's IF samples to if_out + s if_out_stride
  // instead of the chain's IF buffer (nullptr: the IF buffer)
  float2 *if_out = nullptr;
  long long if_out_stride = 0;
  DevBuf<float> d_gain, d_dec, d_hA, d_hB, d_coeff, d_atan, d_if_rms_blk, d_bb_mean_blk, d_bb_rms_blk, d_blk_ph;
  DevBuf<double> d_base, d_raw, d_am0, d_am1, d_a10, d_a11, d_pc0, d_pc1, d_audio, d_ahA, d_ahB, d_pilotcut;
  DevBuf<int> d_tab, d_mpf_ok, d_stereo_blk;
  DevBuf<StreamState> d_state;
  // time-parallel recurrences
  DevBuf<double> d_pll_wfirst;         // start node of every integration wave's first chunk (the fused down-sweep reads it)
  DevBuf<double> d_base_de, d_raw_de, d_pll_nodes, d_pll_G, d_pll_M, d_pll_PQ, d_pll_dstart, d_pll_PQ2, d_pll_dstart2, d_pll_gres,
      d_blk_level, d_agc_M,
      d_dc_G, d_dc_start;
  DevBuf<float> d_agc_nodes, d_agc_G;
  DevBuf<unsigned int> d_agc_tick;      // k_agc_round's last-arrival ticket, one per stream (left at zero by its users)
  DevBuf<unsigned int> d_af_tick;       // ... and k_af_round's
  DevBuf<double> d_af_nodes, d_af_G, d_af_M, d_af_out;   // AmDecoder audio tail, time-parallel form
  DevBuf<int> d_ck_wraps, d_blk_wraps, d_walk_go;
  DevBuf<unsigned long long> d_ck_mask;
  DevBuf<IterFlags> d_flags;
  std::vector<IterFlags> h_flags;
  // block tables: ring of pinned host slots + device slots so that queued
  // asynchronous calls never overwrite a table that is still being copied
  static constexpr int kTabSlots = 8;
  static constexpr int kFirBlk0Off = 1024;                // ... [1024, 2048) first block of every run of the IF filter's matrix-core kernel
  static constexpr int kFusedTile0Off = 512;             // the table's tail: [0, 512) first block of every run of the fused front end, [512, 1024) first macro tile of every run (+ the end)
  static constexpr double kFusedSumWeight = 0.10;        // what a macro tile with per-block partial sums costs more than one without (run_tables)
#ifndef FMR_FE_SPARE_CUS
#define FMR_FE_SPARE_CUS 8
#endif
  // Pipelined chain with many short streams: the front end takes whole workgroups per stream and leaves more than its 8
  // spare compute units (32 streams: 7 x 32 = 224 of 256).  The small kernels beside it then ask for 8 KB of LDS they never
  // touch: a front-end workgroup leaves 7.7 KB of its unit's LDS free, so they can only go to the units it leaves alone
  // instead of sharing one with eight front-end waves (config5: 0.523 -> 0.502 ms per step, the front end 0.273 -> 0.252).
  // With only the 8 spare units (one long stream) the same ballast costs 4% -- the side stream's kernels queue on them.
  static constexpr int kBallastBytes = 8192, kBallastMinSpare = 24;
  static constexpr int kSpareAsideMaxBlocks = 512;   // (run_fm_pll)
  int fe_spare_cus = 0;           // compute units the last front-end launch left alone
  size_t side_ballast() const { return (pipelined && fe_spare_cus >= kBallastMinSpare) ? (size_t)kBallastBytes : 0; }
  static constexpr int kFeSpareCus = FMR_FE_SPARE_CUS;      // CUs the pipelined chain's front end leaves to the kernels beside it
  HostBuf<int> h_tab_all;    // pinned, kTabSlots * tab_ints
  unsigned long long call_seq = 0;      // calls issued
  HostBuf<unsigned long long> h_marks;   // pinned: [0] calls whose table copy has run, [1] pipelined calls whose decoder has finished
  std::vector<StreamState> h_state;
  // last call
  long long last_n_if = 0, last_n_au = 0;
  int last_nb = 0;
  int timing = 0;                       // 0 off, 1 every kernel (diagnostics), 2 the dominant kernel only
  std::vector<KernelTime> dom_times;    // mode 2: ifr_decim events accumulated over calls until queried
  std::vector<KernelTime> ktimes;
  std::vector<KernelTime> trace;        // mode 3
  std::vector<int> trace_stream;        //   0 decoder, 1 side, 2 side2, 3 front end, 4 tail
  Event trace_base;
  static constexpr size_t kMaxTrace = 1u << 16;      // event pairs kept until fmr_get_kernel_trace fetches them (further kernels run untraced)

  ~fmr_chain() {
#ifdef FMR_PLL_TRACE
    if (d_pll_wgr.p && getenv("FMR_PLL_TRACE_OUT")) {
      (void)hipDeviceSynchronize();
      std::vector<unsigned long long> h(d_pll_wgr.n);
      (void)hipMemcpy(h.data(), d_pll_wgr.p, h.size() * 8, hipMemcpyDeviceToHost);
      if (FILE *f = fopen(getenv("FMR_PLL_TRACE_OUT"), "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
    }
#endif
    // a tail stage that was never enqueued (an asynchronous last call nobody synchronised) is dropped, not launched: its
    // output mux would write into the caller's audio buffer, which the caller may have freed by now
    tail_pending = false; walk_pending = false;
    // THE rule of this destructor: every stream of the chain is idle before any member dies.  Then nothing on the device
    // refers to a buffer, an event or a pinned block any more, the owners give everything back, and the order in which
    // the members die does not matter.
    for (hipStream_t st : {stream.p, side.p, side2, tail.p}) if (st) (void)hipStreamSynchronize(st);
    if (env.host_prof && hp_calls)
      fprintf(stderr, "[fmr host prof] calls %lld  front-end %.1f us  tables %.1f us  decoder %.1f us per call\n", hp_calls,
              hp_fe / hp_calls, hp_tab / hp_calls, hp_dec / hp_calls);
  }

  // ---- kernel launch with optional HIP-event timing on the chain's stream ----
  // FMR_FE_STAMPS=1: where on the constant clock a stream reached the end of one of its kernels, in a ring of eight calls
  // (slot 16 (call_seq % kStampCalls) + id behind the workgroup stamps; id 0 / 1: in front of / behind the fused launch; a second
  // ring of the same shape behind the first holds the shader clock [kHz] the stamp in front of the launch measured)
  static constexpr int kStampCalls = 32;
  unsigned long long *stamp_slot(int id) { return d_fe_stamps.p + 3 * (size_t)kMaxFusedWg * S + 16 * (size_t)(call_seq % kStampCalls) + id; }
  void stamp_after(hipStream_t st, const char *name) {
    static const char *const ids[] = {"", "", "deemph_decim", "aud_poly", "pilotcut", "dc_pass1", "fm_out", "pll", "stats", "if_agc", "pll_commit", "pll_finish", "pll_shoot_jac"};
    for (int i = 2; i < 13; i++)
      if (std::strcmp(name, ids[i]) == 0) { hipLaunchKernelGGL(k_fused_stamp, dim3(1), dim3(1), 0, st, stamp_slot(i), 0); return; }
  }
  template <class F>
  void timed_on(hipStream_t st, const char *name, F &&launch_) {
    auto launch = [&] { launch_(); if (d_fe_stamps.p) stamp_after(st, name); };
    // mode 2: only the kernels of the FIR+discriminator stage carry events (two per kernel per call)
    const bool stage_kernel = std::strcmp(name, "ifr_decim") == 0 || std::strcmp(name, "ifr_poly") == 0 ||
                              std::strcmp(name, "ifr_chan") == 0 ||
                              std::strcmp(name, "disc") == 0 || std::strcmp(name, "ifr_fused") == 0 ||
                              std::strcmp(name, "blk_reduce") == 0 ||
                              (mode == FMR_MODE_FM && std::strcmp(name, "fm_block") == 0);   // FM with the IF FIR on
    // mode 4: the same on every fourth call only (two event markers on the decoder stream cost 7-10 us of a 0.56 ms step)
    // mode 5: as mode 4, but the fused front end on EVERY call: it is timed with the events of its own dispatch, which put no
    // markers on the stream
    const bool own_events = !env.evt_markers && std::strcmp(name, "ifr_fused") == 0;
    const bool sampled = timing == 2 || ((timing == 4 || timing == 5) && (call_seq & 3ull) == 0);
    if (stage_kernel && (sampled || (timing == 5 && own_events))) {
      KernelTime kt{name};
      (void)kt.a.create(); (void)kt.b.create();
      if (own_events) {
        ext_a = kt.a; ext_b = kt.b;
        launch();
        ext_a = ext_b = nullptr;
      } else {
        (void)hipEventRecord(kt.a, st);
        launch();
        (void)hipEventRecord(kt.b, st);
      }
      dom_times.push_back(std::move(kt));
      return;
    }
    auto between_markers = [&](std::vector<KernelTime> &into) {
      KernelTime kt{name};
      (void)kt.a.create(); (void)kt.b.create();
      (void)hipEventRecord(kt.a, st);
      launch();
      (void)hipEventRecord(kt.b, st);
      into.push_back(std::move(kt));
    };
    if (timing == 3 && trace.size() < kMaxTrace) {      // trace: every instrumented kernel of every call since the mode was switched on, with its stream
      if (!trace_base) { (void)trace_base.create(); (void)hipEventRecord(trace_base, st); }
      between_markers(trace);
      trace_stream.push_back(st == stream ? 0 : st == side ? 1 : st == side2 ? 2 : 4);
    } else if (timing == 1) between_markers(ktimes);
    else launch();
  }
  template <class F>
  void timed(const char *name, F &&launch) { timed_on(stream, name, launch); }

  // poll a counter in pinned host memory that a one-thread kernel advances (k_signal_host)
  int wait_mark(unsigned long long *mark, unsigned long long need) {
    if (need == 0) return FMR_OK;
    const auto t_lim = std::chrono::steady_clock::now() + std::chrono::seconds(60);
    while (__atomic_load_n(mark, __ATOMIC_ACQUIRE) < need) {
      std::this_thread::yield();
      if (std::chrono::steady_clock::now() > t_lim) { set_err("the GPU did not reach mark %llu within 60 s", need); return FMR_ERR_HIP; }
    }
    return FMR_OK;
  }
  // Equaliser chain: k_mpf4 counts the waits for the AGC kernel it gave up (StreamState::agc_sync_timeouts).  Called by
  // the entry points that synchronise: a new time-out is an error of that call (its audio is void).
  int check_agc_sync() {
    if (!enable_mpf || !d_agc_progress.p) return FMR_OK;
    if (agc_timeouts_seen.size() != (size_t)S) agc_timeouts_seen.assign(S, 0u);
    int bad = -1;
    for (int s = 0; s < S; s++) {
      unsigned v = 0;
      HIPCHK(hipMemcpy(&v, reinterpret_cast<const char *>(d_state.p + s) + offsetof(StreamState, agc_sync_timeouts), sizeof v, hipMemcpyDeviceToHost));
      if (v != agc_timeouts_seen[s]) { agc_timeouts_seen[s] = v; bad = s; }
    }
    if (bad >= 0) {
      set_err("stream %d: the equaliser gave up waiting for the AGC kernel beside it (%u time-outs so far); the audio of this call is void", bad, agc_timeouts_seen[bad]);
      return FMR_ERR_HIP;
    }
    return FMR_OK;
  }
  // create: the shape (plan_create), then the build from it, by stage in the order the call path uses them
  int init(const fmr_config *c, bool channelizer = false, const fmr_mpx_input_config *mpx_in = nullptr);
  int open_device();
  int build_front_end();
  int build_stage_b(const std::vector<float> &fb);
  int build_fused(const std::vector<float> &fa, const std::vector<float> &fb);
  int build_if_filter();
  int build_stats();
  int build_fm();
  int build_nbfm();
  int build_am();
  bool cold = true;                     // no call yet: AGC at its initial gain, PLL unlocked
  int pps_block_base = 0;               // blocks of the call that ran before the part whose PPS events the state holds
  int run_cold_aware(const float2 *d_iq, size_t stride, const uint32_t *block_len, int nb, double *d_aud,
                     size_t astride, uint32_t *audio_len);
  struct TileRuns {      // a tiled kernel's runs: tiles, workgroups per stream, tiles per run (balanced: the first rem runs one longer)
    int tiles = 0, grid = 0, tpw = 0, rem = 0;
    static TileRuns balanced(int tiles, int wgs) { const int g = std::min(wgs, tiles); return {tiles, g, tiles / g, tiles % g}; }
  };
  // Where the IF AGC of a call runs (run_if_stage launches it, or leaves the job to run_fm / run_fm_pll)
  enum class AgcPlace {
    beside_mpf,      // FM with the equaliser: the wave kernel on side2, the equaliser consumes the gains as they are published
    serial,          // FMR_SERIAL=1: the serial kernel on the decoder stream
    aside_after_pll, // FM stereo: Newton rounds on side2, enqueued behind the PLL's first pass (run_fm_pll)
    aside,           // FM mono: Newton rounds on side2, enqueued at once
    in_line,         // NBFM / AM family: Newton rounds on the decoder stream
  };
  // What one call runs (plan_call): every choice that follows from the chain's shape and this call's block lengths, decided
  // before anything is enqueued or any counter moves.  The stages read it and launch; none of them derives a choice again.
  struct CallPlan {
    StageA a = StageA::none;
    StageB b = StageB::none;
    bool b_disc = false;          // stage B carries the discriminator (fused with it, poly5h_disc): the MPX and the block sums
    IfForm fir = IfForm::none;
    int TL = 0;                   // k_fm_block3: tile length (1024 outputs, or the call's longest IF block rounded up to four) ...
    size_t lds_fb = 0;            // ... and its LDS
    ResamplerCounter prev, next;  // the IF resampler's counters before and after the call
    int count_mid = 0;            // stage-A outputs of the call
    int fe_cus = 0;               // compute units the front end's persistent kernels take (pipelined: one per XCD stays free)
    TileRuns fe_runs, fir_runs;   // fused (macro tiles of 384 IF samples) or poly5h_disc (3072), and poly4_disc (3072)
    TileRuns dec16_runs;          // decim16: a contiguous run of 500-output epochs per workgroup (tpw for all but the last)
    int part_from = 0;            // first IF sample whose partial sums k_stats reads (first_part_block; output stage on: 0)
    bool small = false;           // a call of at most kSmallCall IF samples is launch-bound on the host: fewer spare rounds ...
    int c_call = 0;               // ... and shorter PLL chunks (the same rule in both chain forms: N_if only)
    int agc_iters = 0, pll_iters = 0, agc_nc = 0;   // Newton rounds enqueued; chunks of C_AGC samples
    bool iter_on_side = false;    // FM without the equaliser: round flags and AGC start nodes are reset beside the front end
    AgcPlace agc = AgcPlace::in_line;
    bool walk_late = false;       // pipelined chain: the lock logic's walk is enqueued a call late (WalkJob)
    bool spare_aside = false;     // pipelined chain, few blocks: the PLL passes after the second go to the side stream
    bool fir_disc() const { return fir == IfForm::poly4_disc || fir == IfForm::block3_disc; }
    bool fir_tail() const { return fir == IfForm::poly4_disc; }
    bool b_in_tables() const { return b == StageB::fused || b == StageB::poly5h_disc; }   // launched from run_tables (it needs the block table)
  };
  // Deferred work is a job: a plain struct of the values it took from the call that made it, and a member function that
  // takes it by const reference (as TailCtx / tail_stage below); everything else it reads from the chain when it runs.
  struct AgcJob {                 // the IF AGC's Newton rounds + fallback (enqueue_agc)
    const float2 *xin = nullptr; long long x_stride{}; int x_off{};
    const float *nrm_in = nullptr; long long nrm_stride{};   // (non-null: the front end stored |x|^2, not the IF samples)
    long long N_if{}; int nc{}, iters{};
    bool aside{};                 // on side2 beside the decoder stream (FM), else on the decoder stream
    float *gain_out = nullptr;    // null: the recurrence is solved for its state only
    int ginv{};
  };
  struct FePostJob {              // pipelined chain: the front-end stage's end-of-call kernel (launch_fe_post)
    const float2 *d_iq = nullptr; long long stride{}, n_in{}; int count_mid{}, commit{};
    bool pending = false;
  };
  struct WalkJob {                // the lock logic's walk over the blocks of a call (pll_walk)
    const fm_mpx_t *base = nullptr; long long base_stride{};
    BlockTab bt{}; ChunkTab ct{};
    int *ck_wraps = nullptr; unsigned long long *ck_mask = nullptr;   // the creating call's copy of the wrap counts / masks
    int *stereo_blk = nullptr, *walk_go = nullptr;
    size_t ballast{}; bool late{};
  };
  struct HostTab { int *if_off = nullptr, *if_len = nullptr, *au_off = nullptr, *au_len = nullptr, *mpf = nullptr; };
  // values one call's stages hand each other (run() fills the first two groups, every stage adds its part to the third)
  struct CallCtx {
    // ---- what the caller handed in
    const float2 *d_iq = nullptr; size_t stride{};
    const uint32_t *block_len = nullptr; int nb{};
    double *d_aud = nullptr; size_t astride{};
    uint32_t *audio_len = nullptr; long long N_in{};
    unsigned long long out_block0 = 0; // output stage: absolute index of the call's first block
    // ---- this call's table slot: the pinned host copy (its block rows in tab), the device copy
    int *h_tab = nullptr, *d_tab_slot = nullptr; HostTab tab{};
    // ---- what each stage adds.  plan_call / run_front_end:
    long long N_if{};
    CallPlan plan{};
    bool done = false;                 // the front end found nothing to decode
    int par{};                         // this call's slot of the rings the stages hand each other (plain chain: 0, the one buffer of each kind)
    float2 *ifbuf = nullptr; fm_mpx_t *base = nullptr; double *raw = nullptr; FusedPart *part = nullptr; int *stereo_blk = nullptr;
    HaloTable ht{};
    // run_tables:
    long long N_au{}, amA_prev{}, akB_prev{}, an_prev{}, if_stride{};
    bool any_mpf{};
    int nck{}, fused_n_tiles{}, fused_kb_ref{};
    ChunkTab ct{};
    BlockTab bt{};
    float *nrm = nullptr;              // fused front end with the discriminator epilogue: |x|^2 of the IF samples (in the IF slot's memory) instead of the IF samples
    long long nrm_stride{};
    FePostJob fe_post{};
    bool tail_deferred{};              // the previous call's tail stage is still to be enqueued (behind this call's IF filter kernel)
    // run_if_stage:
    const float2 *xin = nullptr; long long x_stride{}; int x_off{};
    const float *disc_gain = nullptr;  // gain sequence the discriminator multiplies in (null: none)
    bool agc_on_side{};
    AgcJob agc{};
    bool agc_deferred{};               // agc is still to be enqueued (run_fm_pll behind the first pass, else run_fm)
    // run_fm:
    hipEvent_t ev_mpx = nullptr;       // recorded where this call's MPX (discriminator output) is complete
    void add_halo(void *buf, long long stride_e, int H, long long N, int words = 2) {   // history to move to the buffer heads at the end of the call (words: 32-bit words per element)
      if (H > 0 && N > 0) ht.d[ht.n++] = HaloDesc{(unsigned *)buf, stride_e * words, H * words, (int)N * words};
    }
  };
  // what the audio tail of one call needs, by value: in the pipelined chain the tail stage is enqueued a call later
  struct TailCtx {
    fm_mpx_t *base = nullptr;
    const float2 *ifbuf = nullptr;     // the call's IF ring slot (the RF monitor reads it) ...
    bool if_nrm = false;               // ... holding |x|^2 (float, from the slot's first word) instead of the IF samples
    double *raw = nullptr;
    int *stereo_blk = nullptr;
    long long N_if{}, N_au{}, a_top0{}, amA_prev{}, akB_prev{}, astride{};
    int nb{}, count_am{}, de_tout{}, dc_nc{}, nch{};
    int au_max{};                // longest audio block of the call
    bool de_fused{}, fin_on_side{}, fin_covers_all{}, agc_on_side{}, mono_enqueued{};
    bool can_split{};            // the mono channel can be enqueued by itself (the shapes the per-channel tail kernels take)
    hipEvent_t ev_mpx = nullptr; // "the MPX of this call is there" (pipelined chain: what a drained tail's mono channel waits for)
    BlockTab bt{};
    double *d_aud = nullptr;
    DcCoef dk{};
    HaloTable ht{};
    unsigned long long seq{};
    OutArgs out{};                     // output stage: the call's positions and its slot of the per-block IF RMS
    const float *out_ifrms = nullptr;
    WsArgs ws{};                       // weak-signal handling: the call's positions
    MpxOutArgs mpxo{};                 // MPX output: the call's positions
  };
  static constexpr int kDeBlock = 256;
  TailCtx tail_job{};
  bool tail_pending = false;
  // Pipelined chain: the lock logic's walk over the blocks of call N (k_pll_finish) is enqueued a call late -- on the side
  // stream behind the tables of call N+1, with the tail of call N whose output mux waits for it (flush_tail), beside the
  // front end of call N+1 -- or by whatever drains the chain.  What the next PLL needs of it, k_pll_commit has committed
  // in call N (kernels_par.hpp): the next call's tables no longer wait for a one-wave walk over 2048 blocks.
  bool walk_pending = false;
  WalkJob walk_job{};
  int pll_walk(const WalkJob &w);
  int flush_walk();
  int walk_par = 0;               // which copy of the PLL's wrap counts / wrap masks / verdict the next call writes
  void tail_channels(const TailCtx &t, hipStream_t st, int ch_base, int nch_l);
  int tail_stage(const TailCtx &t, hipStream_t ts);
  int flush_tail(hipEvent_t gate);
  int enqueue_tail(hipEvent_t gate);
  int plan_call(CallCtx &k);
  int run_front_end(CallCtx &k);
  int launch_chan(hipStream_t st, const float2 *d_iq, long long N_in, long long mA_prev, long long n_prev, int count_mid);
  int finish_front_end_stage(CallCtx &k);
  int run_tables(CallCtx &k);
  void fill_run_blocks(const CallCtx &k, int *blk0, const TileRuns &r, const int *tile0, long long kb_ref, int tile_len);
  int run_if_stage(CallCtx &k);
  int mpxin_stage(CallCtx &k);
  int enqueue_agc(const AgcJob &j, hipEvent_t gate);
  void launch_fe_post(FePostJob &j);
  int run_fm(CallCtx &k);
  int run_fm_pll(CallCtx &k, TailCtx &t);
  int run_nbfm(CallCtx &k);
  int run_am(CallCtx &k);
  int run(const float2 *d_iq, size_t stride, const uint32_t *block_len, int nb, double *d_aud,
          size_t astride, uint32_t *audio_len);
};

// An optional stage is all or nothing: it is built in a local object and moved into the chain only when its init() has
// succeeded.  A failed enable leaves the chain exactly as it was (the local dies with whatever it had allocated), and the
// same call may be made again.
template <class St, class... A>
static int build_stage(St &into, A &&...args) {
  St s;
  if (int rc = s.init(args...)) return rc;
  into = std::move(s);
  return FMR_OK;
}

// The end of every fmr_enable_*, once the configuration has passed and the chain is there and fits: the stage is not on
// yet and no call has been made; then it is built on the chain's device from args (St::init's).  `what` names the stage,
// `first` what it counts from.
template <class St, class... A>
static int enable_stage(const char *fn, fmr_chain *c, St &stage, const char *what, const char *first, A &&...args) {
  if (stage.on) { set_err("%s: the %s of this chain is already enabled", fn, what); return FMR_ERR_BAD_ARG; }
  if (c->call_seq != 0) {
    set_err("%s: the chain has already taken samples (the %s counts from the chain's first %s)", fn, what, first);
    return FMR_ERR_BAD_ARG;
  }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    return build_stage(stage, args...);
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

// The reader's view of stream s of a record ring, after a read, into a *_info: records complete, records overwritten
// unread, the next unread one and how many wait.
template <class Info>
static void ring_info(Info &i, const RecCursor &cur, int s, unsigned long long done) {
  i.records_complete = done;
  i.records_dropped = cur.dropped[s];
  i.first_unread = cur.read[s];
  i.records_ready = done - cur.read[s];
}

template <class T>
static int upload(DevBuf<T> &b, const T *src, size_t n) {
  int rc = b.alloc(n);
  if (rc) return rc;
  if (n) HIPCHK(hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
  return FMR_OK;
}

// A fragments of the banded matrix-core kernel (k_ifr_poly4, shape SH): the row of output position pp = 16 mt + lane % 16
// over window position m = 4 (ks_lo(mt) + i) + lane / 16 holds tap(pp, m) (0 where the row has no tap)
template <class SH, class Tap>
static std::vector<float> poly4_afrag(Tap &&tap) {
  std::vector<float> af((size_t)SH::MT * SH::NK * 64, 0.f);
  for (int mt = 0; mt < SH::MT; mt++)
    for (int i = 0; i < SH::nks(mt); i++)
      for (int l = 0; l < 64; l++) af[((size_t)mt * SH::NK + i) * 64 + l] = tap(16 * mt + (l & 15), 4 * (SH::ks_lo(mt) + i) + (l >> 4));
  return af;
}

// The first block whose partial sums k_stats reads: its walk (kernels.hpp, k_stats) starts at the 64-block group in which
// it has seen 400 non-empty blocks counting from the end; the blocks before it need none.  The same rule as that walk.
static int first_part_block(const int *if_len, int nb) {
  int seen = 0;
  for (int b0 = ((nb - 1) / 64) * 64; b0 > 0; b0 -= 64) {
    for (int b = b0; b < std::min(b0 + 64, nb); b++) seen += if_len[b] != 0;
    if (seen >= 400) return b0;
  }
  return 0;
}

// ---- create, the build step: small helpers, the tables (each a function of what it needs), then the chain stage by stage
template <class T>
static int upload(DevBuf<T> &b, const std::vector<T> &v) { return upload(b, v.data(), v.size()); }
// the window and the twiddles of a Welch stage (welch_tables)
static int upload_welch(const WelchTables &t, DevBuf<float> &d_win, DevBuf<float2> &d_tw) {
  static_assert(sizeof(WelchCpx) == sizeof(float2) && FMR_WINDOW_HANN == kWelchHann && FMR_WINDOW_RECT == kWelchRect &&
                FMR_WINDOW_BLACKMAN_HARRIS == kWelchBlackmanHarris, "welch_plan.hpp's float2 and window kinds");
  if (int rc = upload(d_win, t.win)) return rc;
  return upload(d_tw, reinterpret_cast<const float2 *>(t.tw.data()), t.tw.size());
}

// zeroed buffers for a list of (buffer, count) pairs; the first error ends it
static int alloc_all() { return FMR_OK; }
template <class B, class... Rest>
static int alloc_all(B &b, size_t n, Rest &&...rest) {
  if (int rc = b.alloc(n)) return rc;
  return alloc_all(rest...);
}

// a kernel may ask for up to `bytes` of dynamic LDS (more than the 64 KB every kernel gets)
template <class K>
static int set_dyn_lds(K *kernel, size_t bytes) {
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return FMR_OK;
}

static std::vector<float> to_float(const std::vector<double> &h) { return std::vector<float>(h.begin(), h.end()); }

// stage-B tap rows as d_hB holds them: [LB][TB], or in the fractional-phase form [LT + 1][pitch]
static std::vector<float> hB_rows(const ResamplerDesign &rs, int pitch) {
  if (!rs.LT) return to_float(rs.hB);
  std::vector<float> fb((size_t)(rs.LT + 1) * pitch, 0.f);
  for (int p = 0; p <= rs.LT; p++)
    for (int j = 0; j < rs.TB; j++) fb[(size_t)p * pitch + j] = (float)rs.hB[(size_t)p * rs.TB + j];
  return fb;
}

// stage-A taps in polyphase order [D][qa] (k_ifr_decim2)
static std::vector<float> hpA_table(const std::vector<float> &fa, int D, int qa) {
  std::vector<float> hp((size_t)D * qa, 0.f);
  for (size_t k = 0; k < fa.size(); k++) hp[(k % D) * qa + k / D] = fa[k];
  return hp;
}

// stage-B rows between FMR_POLY_PADZ zeros on either side (k_ifr_poly3 shifts its window into them)
static std::vector<float> hBp_table(const std::vector<float> &fb, const ResamplerDesign &rs) {
  const int TBP = rs.TB + 2 * FMR_POLY_PADZ;
  std::vector<float> hp((size_t)rs.LB * TBP, 0.f);
  for (long long r = 0; r < rs.LB; r++)
    for (int j = 0; j < rs.TB; j++) hp[(size_t)r * TBP + FMR_POLY_PADZ + j] = fb[(size_t)r * rs.TB + j];
  return hp;
}

// the fp16 three-product form (k_ifr_poly5h): A fragments [k-block of 32 taps][row tile][h | l][lane][8] of the taps times 2^ea
static std::vector<_Float16> poly5h_afrag(const std::vector<float> &fb, const StageBLayout &l, int TB, int nkb, int ea) {
  const float sa = std::ldexp(1.0f, ea);
  std::vector<_Float16> ah((size_t)nkb * 3 * 2 * 64 * 8, (_Float16)0.f);
  for (int kb = 0; kb < nkb; kb++)
    for (int mt = 0; mt < 3; mt++)
      for (int ln = 0; ln < 64; ln++)
        for (int e = 0; e < 8; e++) {
          const int pp = 16 * mt + (ln & 15), m = 32 * kb + 8 * (ln >> 4) + e, j = m - l.off[pp];
          if (j < 0 || j >= TB) continue;
          const float t = fb[(size_t)l.phi[pp] * TB + j] * sa;
          const _Float16 hi = (_Float16)t;
          const size_t base = ((((size_t)kb * 3 + mt) * 2) * 64 + ln) * 8 + e;
          ah[base] = hi;
          ah[base + 64 * 8] = (_Float16)(t - (float)hi);
        }
  return ah;
}

// the IF filter (order + 1 taps c) as the 1 : 1 "polyphase" shape 48 / 48 of the banded matrix-core kernel -- one phase,
// window start = output index; tap row h[j'] = c[order - j'] over x[i - order + j'], the lag-0 tap (j' = order) left out:
// the kernel's epilogue (FM -f) or k_fir_finish (48 kHz modes) adds it where the reference has it
template <class SH>
static std::vector<float> fir_afrag(const std::vector<float> &c) {
  const int order = (int)c.size() - 1;
  return poly4_afrag<SH>([&](int pp, int m) { const int j = m - SH::off(pp); return j >= 0 && j < order ? c[order - j] : 0.f; });
}

// a channel bank's stage-A taps c_s[k] = hA[k] exp(+2 pi i ((f_s k) mod F) / F) in double, rounded once: [group][k][g],
// channels beyond S are zero; and per channel f mod F, f D mod F
static void bank_tables(const std::vector<float> &fa, const std::vector<int32_t> &off, unsigned long long F, int D,
                        std::vector<float2> &taps, std::vector<ChanPhase> &ph) {
  const int G = FMR_CB_G, S = (int)off.size(), ng = (S + G - 1) / G, NA = (int)fa.size();
  taps.assign((size_t)ng * NA * G, make_float2(0.f, 0.f));
  ph.resize((size_t)S);
  for (int s = 0; s < S; s++) {
    const long long fl = off[s];
    const unsigned long long fm = (unsigned long long)(((fl % (long long)F) + (long long)F) % (long long)F);
    ph[s] = ChanPhase{fm, (fm * (unsigned long long)D) % F};
    for (int k = 0; k < NA; k++) {
      const double a = 2.0 * M_PI * (double)((fm * (unsigned long long)k) % F) / (double)F;
      const double h = (double)fa[k];
      taps[((size_t)(s / G) * NA + k) * G + (s % G)] = make_float2((float)(h * std::cos(a)), (float)(h * std::sin(a)));
    }
  }
}

// FineTuner(table_size 480 = 48000/100, freq_shift): FineTuner.cpp:25-52 with m_index = 0, phase offset 0
static std::vector<float2> finetuner_table(int freq_shift) {
  const int ts = 480;
  std::vector<float2> t((size_t)ts);
  const double phase_step = 2.0 * M_PI / double(ts);
  for (int i = 0; i < ts; i++) {
    const double phi = (double)(((int64_t)freq_shift * i) % ts) * phase_step;
    t[(size_t)i] = make_float2((float)std::cos(phi), (float)std::sin(phi));
  }
  return t;
}

// (A^LPL)^k, k = 0 .. 64, of the de-emphasis (DeScan::apow)
static std::vector<double> deemph_powers(const Iir1Coef &d) {
  const double a = deemph_step(d);
  std::vector<double> apow(65);
  apow[0] = 1.0;
  for (int k = 1; k <= 64; k++) apow[k] = apow[k - 1] * a;
  return apow;
}

int fmr_chain::init(const fmr_config *c, bool channelizer, const fmr_mpx_input_config *mpx_in) {
  env.load();
  int rc;
  if ((rc = plan_create(*this, c, env, channelizer, mpx_in))) return rc;      // (a refused configuration never opens the device)
  if ((rc = open_device())) return rc;
  if (has_rs && (rc = build_front_end())) return rc;
  if (this->mpx_in) {      // nothing of the IF: no IQ input buffer, no IF buffers, no filter
    if ((rc = build_stage(mpxi, S, max_in, mi_rate, mi_format, mi_gain)) || (rc = build_stats())) return rc;
    return build_fm();
  }
  if ((rc = d_in.alloc((size_t)in_rows() * max_in))) return rc;
  if ((rc = build_if_filter()) || (rc = build_stats())) return rc;
  if (!has_dec) return FMR_OK;
  return mode == FMR_MODE_FM ? build_fm() : mode == FMR_MODE_NBFM ? build_nbfm() : build_am();
}

int fmr_chain::open_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device"); return FMR_ERR_NO_DEVICE; }
  if (cfg.device < 0 || cfg.device >= ndev) { set_err("device %d out of range (%d devices)", cfg.device, ndev); return FMR_ERR_BAD_ARG; }
  HIPCHK(hipSetDevice(cfg.device));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg.device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
  // A pipelined chain has THREE streams ("Three stages in flight"):
  //   stream  the critical chain: front end of call N, PLL of call N, front end of call N+1 ... -- both hold the whole chip
  //           (152 KB of LDS per CU; 1258 one-wave workgroups), so they alternate anyway, and on ONE queue the hand-off
  //           between them is a packet boundary, not an event travelling between two queues (~50 us each way, measured)
  //   side    tables, statistics, the IF AGC, lock logic
  //   tail    the audio tail, a call behind
  // Three, because a process gets four hardware queues from HIP, the host application's own stream included, and more
  // busy queues than that take turns on a pipe in slices of 3.55 ms (measured with four and five busy queues, with and
  // without stream priorities: one process in two then runs at 4-36 ms per step).
  int rc;
  if ((rc = stream.create()) || (rc = side.create())) return rc;
  if (pipelined) {
    side2 = side;
    if ((rc = tail.create())) return rc;
    for (Event &e : ev_fe) if ((rc = e.create(hipEventDisableTiming))) return rc;
  } else {
    if ((rc = side2_own.create())) return rc;
    side2 = side2_own;
  }
  for (Event *e : {&ev_agc, &ev_pll1, &ev_tab, &ev_mono, &ev_disc, &ev_pll, &ev_stats, &ev_fin, &ev_if})
    if ((rc = e->create(hipEventDisableTiming))) return rc;
  return FMR_OK;
}

// IF resampler: the taps of both stages in every layout the chain's forms read, their LDS, the buffers up to the IF
int fmr_chain::build_front_end() {
  const std::vector<float> fa = to_float(rs.hA), fb = hB_rows(rs, hB_pitch);
  int rc;
  if ((rc = upload(d_hA, fa)) || (rc = upload(d_hB, fb))) return rc;
  if (qa && (rc = upload(d_hpA, hpA_table(fa, rs.D, qa)))) return rc;
  if (fe.decim16) {
    using SH16 = Decim16Shape<10, 195>;
    std::vector<unsigned short> fr((size_t)2 * SH16::NKT * 2 * 64 * 8);
    decim16_make_afragA<10, 195>(fa.data(), fr.data());
    if ((rc = upload(d_dec16_afrag, fr)) || (rc = set_dyn_lds(&k_ifr_decim16<10, 195, 0>, SH16::LDS_BYTES)) ||
        (rc = set_dyn_lds(&k_ifr_decim16<10, 195, 1>, SH16::LDS_BYTES))) return rc;
  }
  if ((rc = build_stage_b(fb))) return rc;
  const bool fused = fe.fused != FusedFe::none;
  if (fused && (rc = build_fused(fa, fb))) return rc;
  if ((fused || fe.decim16) && (rc = d_zero16.alloc(4))) return rc;
  if ((rc = alloc_all(d_in_halo, (size_t)in_rows() * H_in, d_mid, (size_t)S * (H_mid + max_mid)))) return rc;
  if (bank) {
    std::vector<float2> taps;
    std::vector<ChanPhase> ph;
    bank_tables(fa, cb_off, cb_F, rs.D, taps, ph);
    if ((rc = upload(d_cb_taps, taps)) || (rc = upload(d_cb_ph, ph))) return rc;
  }
  return FMR_OK;
}

// stage B, whole-phase forms: the position tables every tiled form reads, the padded rows where poly3 fits, and the tap
// fragments of the chain's matrix-core form
int fmr_chain::build_stage_b(const std::vector<float> &fb) {
  if (!poly2_ok) return FMR_OK;      // (poly_frac and poly read d_hB alone)
  const StageBLayout l(rs);
  int rc;
  if ((rc = upload(d_bphi, l.phi)) || (rc = upload(d_boff, l.off)) || (rc = set_dyn_lds(&k_ifr_poly2<512>, 98304))) return rc;
  if (poly3_ok && ((rc = upload(d_hBp, hBp_table(fb, rs))) || (rc = set_dyn_lds(&k_ifr_poly3<384, StageBLayout::Q3>, 98304)))) return rc;
  auto tap = [&](int row, int j) { return j >= 0 && j < rs.TB ? fb[(size_t)row * rs.TB + j] : 0.f; };
  if (fe.b == StageB::poly5h) {
    if ((rc = upload(d_afrag5h, poly5h_afrag(fb, l, rs.TB, poly5h_nkb, poly5h_ea))) || (rc = set_dyn_lds(&k_ifr_poly5h<48, 125>, poly5h_lds)) ||
        (rc = set_dyn_lds(&k_ifr_poly5h<48, 125, Poly5hDiscEpi>, poly5h_lds))) return rc;
  } else if (fe.b == StageB::poly4_am) {
    using SH = Poly4Shape<48, 128, 214>;
    if ((rc = upload(d_afrag, poly4_afrag<SH>([&](int pp, int m) { return tap(l.phi[pp % 3], m - SH::off(pp)); }))) ||
        (rc = set_dyn_lds(&k_ifr_poly4<48, 128, 214>, 98304))) return rc;
  } else if (fe.b == StageB::poly4) {
    using SH = Poly4Shape<48, 125, 210>;
    if ((rc = upload(d_afrag, poly4_afrag<SH>([&](int pp, int m) { return tap(l.phi[pp], m - l.off[pp]); }))) ||
        (rc = set_dyn_lds(&k_ifr_poly4<48, 125, 210>, 98304))) return rc;
  }
  return FMR_OK;
}

// fused front end (stage B is poly4's 48 / 125 / 210 here): both stages' taps as fp16 fragments, the tap row of position
// 47, and per workgroup the fp32 copies of mid samples beyond fp16's range -- the one size that follows from the device
int fmr_chain::build_fused(const std::vector<float> &fa, const std::vector<float> &fb) {
  std::vector<unsigned short> fr((size_t)2 * 8 * 2 * 64 * 8), frb((size_t)3 * 9 * 2 * 64 * 8);
  fused_make_afragA<kFusedD, kFusedNA>(fa.data(), fr.data());
  fused_hB_inv_scale = fused_make_afragB(fb.data(), frb.data());
  constexpr int kL = FusedShape<kFusedD, kFusedNA>::LDS_BYTES;
  int rc;
  if ((rc = upload(d_hB_last, fb.data() + (size_t)((47 * rs.MB) % rs.LB) * rs.TB, (size_t)rs.TB)) ||
      (rc = upload(d_fused_afragA, fr)) || (rc = upload(d_fused_afragB, frb)) ||
      (rc = set_dyn_lds(&k_ifr_fused<kFusedD, kFusedNA, 0, 0>, kL)) || (rc = set_dyn_lds(&k_ifr_fused<kFusedD, kFusedNA, 1, 0>, kL)) ||
      (rc = d_fused_mid32.alloc((size_t)std::max(std::max(n_cu, S), 256) * 2 * FusedShape<kFusedD, kFusedNA>::MIDR))) return rc;
  if (env.fe_stamps && (rc = d_fe_stamps.alloc(3 * (size_t)kMaxFusedWg * S + 2 * kStampCalls * 16))) return rc;
  return FMR_OK;
}

// IF buffers (one per ring slot on a pipelined chain) and the IF filter: its taps, and its matrix-core form's fragments
int fmr_chain::build_if_filter() {
  int rc;
  for (int q = 0; q < (pipelined ? kPipe : 1); q++)
    if ((rc = (q ? d_if_pp[q] : d_if).alloc((size_t)S * (H_if + max_if)))) return rc;
  last_if = d_if.p;
  if (!has_dec) return FMR_OK;
  if ((rc = upload(d_coeff, filter))) return rc;
  if (fir_enable && (rc = d_fir.alloc((size_t)S * max_if))) return rc;
  if (fe.fir == IfForm::poly4_disc) {      // FM -f: lags 1 .. 126, lag 0 and the discriminator in the epilogue (Poly4FirDiscEpi)
    if ((rc = upload(d_afrag_fir_fm, fir_afrag<Poly4Shape<48, 48, 127>>(filter))) ||
        (rc = set_dyn_lds(&k_ifr_poly4<48, 48, 127, 2, Poly4FirDiscEpi>, 98304))) return rc;
  } else if (fe.fir == IfForm::poly4_finish) {      // AM / DSB / NBFM (round 6: k_fm_block2 took 0.139 ms per 2.1 M IF samples, a fifth of the AM step)
    if (ntaps == 255) {
      if ((rc = upload(d_afrag_fir, fir_afrag<Poly4Shape<48, 48, 255>>(filter))) || (rc = set_dyn_lds(&k_ifr_poly4<48, 48, 255, 1>, 98304))) return rc;
    } else {
      if ((rc = upload(d_afrag_fir, fir_afrag<Poly4Shape<48, 48, 127>>(filter))) || (rc = set_dyn_lds(&k_ifr_poly4<48, 48, 127, 2>, 98304))) return rc;
    }
  }
  return FMR_OK;
}

// per-stream state, the call tables' slots, round flags; with a decoder the IF AGC, the discriminator's outputs, the
// partial sums of the epilogues that leave block sums, and the per-block statistics
int fmr_chain::build_stats() {
  int rc;
  h_state.assign(S, StreamState{});
  for (auto &st : h_state) {
    st.agc_gain = 1.0f;
    st.pll_freq = (19000.0 / kFmRate) * 2.0 * M_PI;   // PilotPhaseLock.cpp:40
    st.af_gain = 1.0;
  }
  if ((rc = upload(d_state, h_state))) return rc;
  if ((rc = h_tab_all.alloc(kTabSlots * tab_ints, hipHostMallocDefault))) return rc;
  // The marks are written by one-thread kernels and polled by the host while more work is queued behind them: COHERENT
  // (fine-grained) host memory, so that the store leaves the GPU when it is made.  With the default flags the line may sit
  // in the GPU's L2 until some later system-scope release writes it back, and a host that waits for a mark sees it
  // milliseconds late (measured: one process in two ran at 4-36 ms per step, in multiples of 3.55 ms).
  if ((rc = h_marks.alloc(2, hipHostMallocCoherent))) return rc;
  h_marks.p[0] = h_marks.p[1] = 0;
  h_flags.assign(S, IterFlags{});
  if ((rc = alloc_all(d_tab, (size_t)kTabSlots * tab_ints, d_flags, (size_t)S))) return rc;
  if (!has_dec) return FMR_OK;
  const size_t SB = (size_t)S * max_blocks;
  if (!mpx_in &&      // (the IF AGC's buffers: an MPX input has no IF)
      (rc = alloc_all(d_agc_nodes, (size_t)S * (max_agc_nc + 1), d_agc_tick, (size_t)S, d_af_tick, (size_t)S,
                      d_agc_G, (size_t)S * max_agc_nc, d_agc_M, (size_t)S * max_agc_nc, d_gain, (size_t)S * max_if,
                      d_blk_ph, SB * 2))) return rc;
  if ((rc = alloc_all(d_dec, (size_t)S * max_if, d_if_rms_blk, SB, d_bb_mean_blk, SB, d_bb_rms_blk, SB,
                      d_mpf_ok, SB, d_stereo_blk, SB))) return rc;
  const bool tiled_epi = fe.poly5h_disc || fe.fir == IfForm::poly4_disc;
  if ((fe.fused != FusedFe::none || tiled_epi) && (rc = d_fused_part.alloc((size_t)S * 3 * (max_if / 384 + 20)))) return rc;
  if (tiled_epi && (rc = d_run_ph.alloc((size_t)S * 2 * kMaxFusedWg))) return rc;
  return FMR_OK;
}

// FM: the ring slots behind the discriminator, the pilot PLL's multiple-shooting buffers, the audio tail, the equaliser
int fmr_chain::build_fm() {
  int rc;
  float atan_tab[257];
  make_fast_atan_table(atan_tab);
  if ((rc = upload(d_de_pow, deemph_powers(deemph))) || (rc = upload(d_ahA, ars.hA)) || (rc = upload(d_ahB, ars.hB)) ||
      (rc = upload(d_pilotcut, k_jj1bdx_48khz_fmaudio, (size_t)n_pilotcut)) ||   // FmDecode.cpp:48-49
      (rc = upload(d_atan, atan_tab, (size_t)257))) return rc;
  de_scan.apow = d_de_pow.p;
  const size_t SB = (size_t)S * max_blocks, mpx = (size_t)S * (H_b + max_if);
  for (int q = 0; q < (pipelined ? kPipe : 1); q++) {
    if ((rc = alloc_all(q ? d_base_pp[q] : d_base, mpx, q ? d_raw_pp[q] : d_raw, mpx))) return rc;
    if (q && d_fused_part.p && (rc = d_part_pp[q].alloc(d_fused_part.n))) return rc;
    if (q && (rc = d_stereo_pp[q].alloc(SB))) return rc;
  }
  const size_t copies = pipelined ? 2 : 1;      // (pipelined chain: two copies of the wrap counts and masks, see walk_par)
  const size_t max_grp = max_ck / FMR_NODE_GRP + 2, max_grp2 = (size_t)pll_tick2_per_stream, waves = max_ck / 64 + 2;
  if ((rc = alloc_all(d_base_de, (size_t)S * (H_a + max_if), d_raw_de, (size_t)S * (H_a + max_if),
                      d_pll_nodes, (size_t)S * (max_ck + 1) * 7, d_pll_G, (size_t)S * max_ck * 9, d_pll_M, (size_t)S * max_ck * 49,
                      d_ck_wraps, ck_copy * copies, d_walk_go, (size_t)S * 2,
                      d_pll_PQ, (size_t)S * max_grp * 56, d_pll_dstart, (size_t)S * max_grp * 7, d_pll_gres, (size_t)S * max_grp * 8,
                      d_pll_wgr, (size_t)S * waves * 8,      // (x 8: room for the FMR_PLL_TRACE records)
                      d_pll_PQ2, (size_t)S * max_grp2 * 56, d_pll_dstart2, (size_t)S * max_grp2 * 7, d_pll_pre, (size_t)S * max_grp * 56,
                      d_pll_te, (size_t)S * max_grp * FMR_TREE_SINK * FMR_MAP,      // (17 MB at 2^27 samples a call)
                      d_pll_wfirst, (size_t)S * waves * 7, d_pll_sync, (size_t)S,      // (zeroed here; the kernels leave it zeroed)
                      d_pll_tick2, (size_t)S * max_grp2, d_ck_mask, ck_copy * mask_words * copies,
                      d_blk_wraps, SB, d_blk_level, SB))) return rc;
  const size_t dc = (size_t)S * 2 * max_dc_nc * 2;
  if ((rc = alloc_all(d_dc_G, dc, d_dc_start, dc, d_am0, (size_t)S * (H_am + max_amid), d_am1, (size_t)S * (H_am + max_amid),
                      d_a10, (size_t)S * (H_pc + max_au), d_a11, (size_t)S * (H_pc + max_au), d_pc0, (size_t)S * max_au,
                      d_pc1, (size_t)S * max_au, d_audio, (size_t)S * 2 * max_au))) return rc;
  // MultipathFilter: the reference tap at one, the rest at zero
  std::vector<float2> cf((size_t)S * mpf_N, make_float2(0.f, 0.f));
  for (int s = 0; s < S; s++) cf[(size_t)s * mpf_N + mpf_ref] = make_float2(1.f, 0.f);
  if ((rc = upload(d_mpf_coeff, cf)) || (rc = d_mpf_state.alloc((size_t)S * mpf_N))) return rc;
  if (enable_mpf && (rc = alloc_all(d_mpf, (size_t)S * max_if, d_agc_progress, (size_t)S))) return rc;
  return FMR_OK;
}

int fmr_chain::build_nbfm() {
  int rc;
  if ((rc = upload(d_pilotcut, k_jj1bdx_48khz_nbfmaudio, (size_t)n_pilotcut))) return rc;
  return alloc_all(d_base, (size_t)S * (H_b + max_if), d_audio, (size_t)S * max_au);
}

// AM family: the SSB modes' mixers, and the time-parallel audio tail (DC block and audio AGC in chunks of C_AM)
int fmr_chain::build_am() {
  int rc;
  if (ssb_like) {      // AmDecode.cpp:83-90: USB / WSPR mix down 1500 Hz in front of the filter and up behind it, LSB the other way, CW up 500 Hz behind it
    const int pre = mode == FMR_MODE_LSB ? 15 : mode == FMR_MODE_CW ? 0 : -15, post = mode == FMR_MODE_LSB ? -15 : mode == FMR_MODE_CW ? 5 : 15;
    if (pre && (rc = upload(d_ft_pre, finetuner_table(pre)))) return rc;
    if ((rc = upload(d_ft_post, finetuner_table(post)))) return rc;
  }
  const size_t nc = max_if / C_AM + 2;
  return alloc_all(d_base, (size_t)S * max_if, d_audio, (size_t)S * max_au, d_dc_G, (size_t)S * 2 * nc * 2,
                   d_dc_start, (size_t)S * 2 * nc * 2, d_af_nodes, (size_t)S * (nc + 1), d_af_G, (size_t)S * nc,
                   d_af_M, (size_t)S * nc, d_af_out, (size_t)S * max_if);
}

// stage A of every channel for count_mid outputs from mA_prev on (k_ifr_chan)
int fmr_chain::launch_chan(hipStream_t st, const float2 *d_iq, long long N_in, long long mA_prev, long long n_prev, int count_mid) {
  constexpr int G = FMR_CB_G;
  const long long top0 = (long long)rs.D * mA_prev + rs.ca() - n_prev;
  const unsigned long long N0 = (unsigned long long)rs.D * (unsigned long long)mA_prev + (unsigned long long)rs.ca();
  const unsigned long long nmod0 = N0 % cb_F;
  const size_t tail = sizeof(float2) * (size_t)(rs.NA - 1), per_out = sizeof(float2) * (size_t)rs.D;
  auto go = [&](auto bl_tag) {
    constexpr int BL = decltype(bl_tag)::value;
    const dim3 grid((unsigned)((count_mid + BL - 1) / BL), (unsigned)((S + G - 1) / G));
    hipLaunchKernelGGL((k_ifr_chan<BL, G>), grid, dim3(BL), per_out * BL + tail, st, d_iq, N_in, d_in_halo.p, H_in,
                       d_cb_taps.p, rs.NA, rs.D, top0, count_mid, d_mid.p, (long long)(H_mid + max_mid), H_mid, d_cb_ph.p, S,
                       nmod0, cb_F);
  };
  cb_forms |= FMR_CB_MODTAP;
  timed_on(st, "ifr_chan", [&] {
    if (256 * per_out + tail <= 60000) go(std::integral_constant<int, 256>{});
    else if (128 * per_out + tail <= 60000) go(std::integral_constant<int, 128>{});
    else go(std::integral_constant<int, 64>{});
  });
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// A chain's first call starts from the initial AGC gain and an unlocked PLL; over that transient the Newton
// iterations of the time-parallel recurrences diverge and the serial kernels take over -- 2 s for a 2048-block
// call.  A call is by construction equal to its blocks processed one after the other, so a long first call is
// cut after ~0.8 s of signal: the head pays the serial price (~0.1 s), the rest starts locked and runs parallel.
int fmr_chain::run_cold_aware(const float2 *d_iq, size_t stride, const uint32_t *block_len, int nb, double *d_aud,
                              size_t astride, uint32_t *audio_len) {
  const bool was_cold = cold;
  pps_block_base = 0;
  auto plain = [&]() { const int rc0 = run(d_iq, stride, block_len, nb, d_aud, astride, audio_len); if (rc0 == FMR_OK) cold = false; return rc0; };
  if (!was_cold || mode != FMR_MODE_FM || !has_rs || nb < 2) return plain();
  const double target = 0.8 * cfg.input_rate;
  double total = 0;
  for (int b = 0; b < nb; b++) total += block_len[b];
  if (total < 2.0 * target) return plain();
  size_t in_off = 0;
  int k = 0;
  while (k < nb - 1 && (double)in_off < target) in_off += block_len[k++];
  if (in_fmt != 0 && (in_off * (size_t)in_bps) % 16 != 0) return plain();
  std::vector<uint32_t> al((size_t)nb, 0);
  int rc = run(d_iq, stride, block_len, k, d_aud, astride, al.data());
  if (rc) return rc;
  cold = false;
  // The head (< 0.8 s of signal from a cold PLL) cannot hold a PPS event: the first one needs the lock (0.5 s) plus
  // 19000 pilot periods (1 s).  The state keeps the tail's events; their block index is reported relative to the call.
  pps_block_base = k;
  size_t au_off = 0;
  for (int b = 0; b < k; b++) au_off += al[b];
  const float2 *iq2 = reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(d_iq) + in_off * (size_t)in_bps);
  rc = run(iq2, stride, block_len + k, nb - k, d_aud ? d_aud + au_off : nullptr, astride, al.data() + k);
  if (rc) return rc;
  if (audio_len) for (int b = 0; b < nb; b++) audio_len[b] = al[b];
  return FMR_OK;
}

int fmr_chain::run(const float2 *d_iq, size_t stride, const uint32_t *block_len, int nb, double *d_aud,
                   size_t astride, uint32_t *audio_len) {
  if (nb < 1 || nb > max_blocks) { set_err("n_blocks %d outside 1..%d", nb, max_blocks); return FMR_ERR_CAPACITY; }
  long long N_in = 0;
  for (int b = 0; b < nb; b++) {
    if (block_len[b] > cfg.max_block_len) { set_err("block %d longer than max_block_len", b); return FMR_ERR_CAPACITY; }
    N_in += block_len[b];
  }
  if (in_fmt != 0 && ((stride * (size_t)in_bps) % 16 != 0 || ((uintptr_t)d_iq % 16) != 0)) {
    set_err("raw-format input: the buffer and the stream stride must be 16-byte aligned");
    return FMR_ERR_BAD_ARG;
  }
  HIPCHK(hipSetDevice(cfg.device));
  const auto hp0 = std::chrono::steady_clock::now();
  auto hp1 = hp0, hp2 = hp0;
  struct HostProf {
    fmr_chain *c; const std::chrono::steady_clock::time_point &t0, &t1, &t2;
    ~HostProf() {
      if (!c->env.host_prof) return;
      const auto t3 = std::chrono::steady_clock::now();
      c->hp_fe += std::chrono::duration<double, std::micro>(t1 - t0).count();
      c->hp_tab += std::chrono::duration<double, std::micro>(t2 - t1).count();
      c->hp_dec += std::chrono::duration<double, std::micro>(t3 - t2).count();
      c->hp_calls++;
    }
  } host_prof_guard{this, hp0, hp1, hp2};
  ktimes.clear();
  // Table slot ring: the slot is free once the copy kernel of the call that used it kTabSlots calls ago has run.
  // That kernel's successor writes a counter into pinned host memory which is polled here -- hipEventSynchronize
  // would block until the newest signal of the side stream at call time (most of the PREVIOUS call) and stop the
  // host from enqueueing ahead (measured).
  if (rds.on) rds.drain();                 // (what the device has finished: keeps the host decoders a call or two behind)
  call_seq++;
  const int slot = (int)(call_seq % kTabSlots);
  if (int rcw = wait_mark(&h_marks.p[0], call_seq > (unsigned long long)kTabSlots ? call_seq - kTabSlots : 0)) return rcw;
  // ---- the stages of one call share their per-call values through CallCtx (run_front_end ... run_am below)
  CallCtx k{};
  k.d_iq = d_iq; k.stride = stride; k.block_len = block_len; k.nb = nb; k.d_aud = d_aud; k.astride = astride;
  k.audio_len = audio_len; k.N_in = N_in;
  if (iqc.on && N_in > 0) if (int rc = iqc_stage(k.d_iq, k.stride, N_in)) return rc;         // (FMR_IQC_ACT: the blanker and every reader below take the corrected rows)
  if (this->nb.on && N_in > 0) if (int rc = nb_stage(k.d_iq, k.stride, N_in)) return rc;     // (FMR_NB_ACT: every reader below takes the blanked rows)
  k.h_tab = h_tab_all.p + (size_t)slot * tab_ints;
  k.d_tab_slot = d_tab.p + (size_t)slot * tab_ints;
  k.tab = HostTab{k.h_tab, k.h_tab + max_blocks, k.h_tab + 2 * max_blocks, k.h_tab + 3 * max_blocks, k.h_tab + 4 * max_blocks};
  if (out.on) { k.out_block0 = out.block; out.block += (unsigned long long)nb; }   // (every block handed in counts, empty ones too)
  if (int rc = run_front_end(k)) return rc;
  if (k.done) return flush_tail(nullptr);     // (nothing to decode: a pending tail refers to a table slot this call's successors will reuse)
  k.base = base_slot(k.par); k.raw = raw_slot(k.par); k.part = part_slot(k.par); k.stereo_blk = stereo_slot(k.par);
  hp1 = std::chrono::steady_clock::now();
  if (int rc = run_tables(k)) return rc;
  hp2 = std::chrono::steady_clock::now();
  if (int rc = mpx_in ? mpxin_stage(k) : run_if_stage(k)) return rc;
  if (int rc = (mode == FMR_MODE_FM) ? run_fm(k) : (mode == FMR_MODE_NBFM) ? run_nbfm(k) : run_am(k)) return rc;
  if (k.ht.n)      // (pipelined chain: the tail stage has taken the table with it, flush_tail)
    timed("shift_halo", [&] { hipLaunchKernelGGL(k_shift_halo<256>, dim3(k.ht.n, S), dim3(256), 0, stream, k.ht); });
  if (pipelined) { ring_prev = k.par; ring_prev_n = k.N_if; }
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// the FMR_FE_* bit of every form, in the order of StageA / StageB (a bank's stage A sets none: FMR_CB_*)
static constexpr unsigned kFeBitA[] = {0, 0, 0, FMR_FE_FUSED, FMR_FE_DECIM16, FMR_FE_DECIM2_16, FMR_FE_DECIM2_24, FMR_FE_DECIM};
static constexpr unsigned kFeBitB[] = {0, FMR_FE_FUSED, FMR_FE_POLY5H_DISC, FMR_FE_POLY5H, FMR_FE_POLY4_AM, FMR_FE_POLY4,
                                       FMR_FE_POLY3, FMR_FE_POLY2, FMR_FE_POLY_FRAC, FMR_FE_POLY};

// The kernel forms of one call, from its IF block lengths, the input's alignment and the forms plan_create() allowed.  Fills the
// IF block table and nothing else: a call refused here leaves the chain as it found it.
int fmr_chain::plan_call(CallCtx &k) {
  CallPlan &p = k.plan;
  p = CallPlan{};
  p.prev = p.next = rsc;
  k.N_if = 0;
  bool short_blk = false;      // a non-empty IF block shorter than 128 samples: the tiled forms' epilogues take none
  int tl = 4;
  unsigned long long mi_f = mpxi.frames;      // MPX input: the count law over the frames, from a copy of the counter
  for (int b = 0; b < k.nb; b++) {
    int n;
    if (mpx_in) {
      n = (int)(mpxi.samples_after(mi_f + k.block_len[b]) - mpxi.samples_after(mi_f));
      mi_f += k.block_len[b];
    } else
      n = has_rs ? (int)p.next.advance(rs, k.block_len[b]) : (int)k.block_len[b];
    k.tab.if_off[b] = (int)k.N_if;
    k.tab.if_len[b] = n;
    k.N_if += n;
    short_blk |= n != 0 && n < 128;
    tl = std::max(tl, (n + 3) & ~3);
  }
  const long long N_if = k.N_if;
  p.count_mid = (int)(p.next.mA - p.prev.mA);
  const bool tiled = has_dec && !env.serial && !short_blk;
  // Pipelined chain: the front end leaves one CU of every XCD free.  A workgroup is dispatched inside the XCD its index
  // maps to, and the kernels that run beside the front end -- lock logic (32 KB of LDS), the DC block's node pass (213
  // VGPRs), the spare PLL rounds -- do not fit beside a 152 KB workgroup: on an XCD the front end fills they wait for
  // it to end (measured: the lock logic 250 instead of 55 us, and the next PLL pass behind it).
  const int fe_cus = p.fe_cus = pipelined ? std::max(8, n_cu - kFeSpareCus) : n_cu;
  p.part_from = k.tab.if_off[out.on ? 0 : first_part_block(k.tab.if_len, k.nb)];
  p.small = N_if <= kSmallCall;
  p.agc_nc = (int)((N_if + C_AGC - 1) / C_AGC);
  p.c_call = (p.small && env.x_cpll == 0) ? kCPllSmall : c_pll;
  p.agc_iters = (mode == FMR_MODE_FM && p.small) ? 3 : K_AGC_ITERS;     // one spare round instead of two to four; if that is not
  p.pll_iters = p.small ? 3 : K_PLL_ITERS;                              // enough the serial kernel runs over these few thousand samples
  p.iter_on_side = mode == FMR_MODE_FM && !env.serial && !enable_mpf;
  p.agc = (enable_mpf && !env.serial && mode == FMR_MODE_FM) ? AgcPlace::beside_mpf
        : (env.serial || enable_mpf) ? AgcPlace::serial
        : mode != FMR_MODE_FM ? AgcPlace::in_line
        : stereo ? AgcPlace::aside_after_pll : AgcPlace::aside;
  p.walk_late = pipelined && !env.pll_v1 && !env.serial;
  // Pipelined chain, streams of few blocks: the PLL passes after the second -- which a call in lock does not need, and which
  // then cost five launches that read a flag and leave, ~25 us between this call's accepted pass and the next call's front
  // end -- go to the side stream, in front of the lock logic that waits for them anyway (32 streams x 64 blocks: 0.503 ->
  // 0.478 ms per step).  When they are needed they run beside the next front end; nothing of that call reads what they
  // write before its tables, which are behind the lock logic on the same stream.  Not with one long stream: there the side
  // stream is as long as the step already, and five more launches on it hold the next call's tables back (0.517 -> 0.539).
  p.spare_aside = pipelined && !env.pll_v1 && k.nb <= (env.x_spare_aside >= 0 ? env.x_spare_aside : kSpareAsideMaxBlocks);
  if (mpx_in) {
    if ((size_t)N_if > max_if) { set_err("internal capacity exceeded"); return FMR_ERR_CAPACITY; }      // (StageA::none / StageB::none: mpxin_stage is the front end)
  } else if (!has_rs) {
    p.a = StageA::pass;
  } else {
    if ((size_t)p.count_mid > max_mid || (size_t)N_if > max_if) { set_err("internal capacity exceeded"); return FMR_ERR_CAPACITY; }
    const bool aligned = ((uintptr_t)k.d_iq % 16) == 0 && (k.stride % 2) == 0;
    if (fe.fused != FusedFe::none && tiled && N_if >= 4 * 384 && p.count_mid >= H_mid && aligned) {
      // Fused front end (stage A + stage B + discriminator in one persistent kernel) when this call is long enough and
      // its blocks are not tiny; any other call takes the three-kernel path -- both keep the same carried state.
      p.a = StageA::fused;
      p.b = StageB::fused;
      p.b_disc = fe.fused == FusedFe::disc;
      const long long P_first = p.prev.kB / 48, P_last = (p.prev.kB + N_if - 1) / 48;
      TileRuns &r = p.fe_runs;
      r.tiles = (int)(P_last / 8 - P_first / 8 + 1);
      const int cus = (pipelined && env.fe_cus > 0) ? std::min(env.fe_cus, n_cu) : fe_cus;
      const int wg_per_stream = std::max(1, std::min(kFusedTile0Off - 1, cus / S));
      // (ceil(n / grid) macro tiles for all but the last workgroup.  Balanced runs -- n mod grid workgroups with one tile more --
      // were measured in round 6: 248 instead of 245 workgroups at 2^27 samples, and the launch 5 us LONGER in the chain: the
      // three compute units more that the uneven split leaves free serve the kernels beside it)
      r.tpw = (r.tiles + wg_per_stream - 1) / wg_per_stream;
      r.grid = (r.tiles + r.tpw - 1) / r.tpw;
      if ((size_t)r.tiles * 3 * S > d_fused_part.n) { set_err("internal capacity exceeded (fused tiles)"); return FMR_ERR_CAPACITY; }
      if ((size_t)r.grid * S * 2 * FusedShape<kFusedD, kFusedNA>::MIDR > d_fused_mid32.n) { set_err("internal capacity exceeded (fused workgroups)"); return FMR_ERR_CAPACITY; }
    } else {
      if (p.count_mid > 0)
        p.a = bank ? StageA::bank
            : (fe.decim16 && p.count_mid >= 4 * 500 && aligned) ? StageA::decim16
            : qa == 24 ? StageA::decim2_24 : qa == 16 ? StageA::decim2_16 : StageA::decim;
      if (p.a == StageA::decim16) {
        TileRuns &r = p.dec16_runs;
        r.tiles = (p.count_mid + Decim16Shape<10, 195>::ME - 1) / Decim16Shape<10, 195>::ME;
        const int wgs = std::max(1, fe_cus / S);
        r.tpw = (r.tiles + wgs - 1) / wgs;
        r.grid = (r.tiles + r.tpw - 1) / r.tpw;
      }
      if (p.a == StageA::decim && in_fmt != 0) { set_err("input_format != cf32 needs the v2 front-end kernel (decimation ratio out of its range)"); return FMR_ERR_UNSUPPORTED; }
      if (fe.poly5h_disc && tiled && N_if >= 3072 && p.count_mid > 0) {
        // R8B class: the dense stage B carries the discriminator epilogue (it needs the block table: launched from
        // run_tables), in contiguous runs of stage-B tiles (64 periods = 3072 IF samples) per workgroup.  Balanced runs: ceil(tiles / workgroups) for everybody left 16 of 256 compute units
        // idle at 2^27 samples per call and put seven tiles WITH partial sums on the workgroups that end the launch.
        p.b = StageB::poly5h_disc;
        p.b_disc = true;
        const long long P_first = p.prev.kB / 48, P_last = (p.prev.kB + N_if - 1) / 48;
        p.fe_runs = TileRuns::balanced((int)((P_last - P_first) / 64 + 1), std::max(1, std::min(kFusedTile0Off - 1, fe_cus / S)));
        if ((size_t)8 * p.fe_runs.tiles * 3 * S > d_fused_part.n || (size_t)p.fe_runs.grid * 2 * S > d_run_ph.n) { set_err("internal capacity exceeded (stage-B tiles)"); return FMR_ERR_CAPACITY; }
      } else if (N_if > 0) {
        p.b = fe.b;
      }
    }
  }
  if (has_dec && !mpx_in && !(mode == FMR_MODE_FM && !fir_enable && !env.serial)) {
    // (FM without the IF FIR: the block RMS is taken inside the discriminator kernel, IfForm::none)
    p.TL = std::min(1024, tl);
    p.lds_fb = sizeof(float2) * (4 * (size_t)fm_block3_plane(ntaps - 1, p.TL) + ((size_t)ntaps + 4) / 2 + (size_t)(ntaps - 1) + p.TL);
    const bool blocked = fir_enable && ntaps >= 2 && p.lds_fb <= 60000 && !env.serial;
    if (blocked && mode == FMR_MODE_FM && !enable_mpf)
      p.fir = (fe.fir == IfForm::poly4_disc && tiled && N_if >= 3072) ? IfForm::poly4_disc : IfForm::block3_disc;
    else if (blocked && mode == FMR_MODE_FM) p.fir = IfForm::block3;
    else if (blocked && fe.fir == IfForm::poly4_finish && N_if >= 48) p.fir = IfForm::poly4_finish;
    else p.fir = blocked ? IfForm::block2 : IfForm::block;
  }
  if (p.fir == IfForm::poly4_disc) {
    // FM -f on the matrix cores: contiguous runs of 3072-output tiles per workgroup (call-relative).  Two workgroups share a
    // compute unit: balanced runs keep all of them busy, where ceil(tiles / slots) for everybody left 46 of 256 units idle at
    // 2^27 samples per call.
    p.fir_runs = TileRuns::balanced((int)((N_if - 1) / 3072 + 1), std::max(1, std::min(kMaxFusedWg - kFirBlk0Off, 2 * n_cu / S)));
    if ((size_t)8 * p.fir_runs.tiles * 3 * S > d_fused_part.n || (size_t)p.fir_runs.grid * 2 * S > d_run_ph.n) { set_err("internal capacity exceeded (IF filter tiles)"); return FMR_ERR_CAPACITY; }
  }
  return FMR_OK;
}

// IfResampler (or the pass-through copy): input -> IF buffer, input history, first halo entries
int fmr_chain::run_front_end(CallCtx &k) {
  if (int rc = plan_call(k)) return rc;
  const CallPlan &p = k.plan;
  const long long N_if = k.N_if, N_in = k.N_in, mA_prev = p.prev.mA, kB_prev = p.prev.kB;
  const int count_mid = p.count_mid;
  fe_forms_a |= kFeBitA[(int)p.a];
  fe_forms_b |= kFeBitB[(int)p.b];
  fe_spare_cus = 0;
  hipStream_t fes = stream;      // (pipelined chain too: the front end alternates with the PLL stage on the decoder stream)
  k.par = 0;
  if (has_rs) {
    rsc = p.next;
    // Cross-call pipelining: this call's front end (its own stream, its own slot of the IF / MPX / partial-sum ring) runs
    // beside the PLL stage of the call before it and the audio tail of the call before that.  The slot was last read by the
    // tail of the call kPipe calls ago: the host polls a counter that a one-thread kernel at the end of every tail writes
    // into pinned host memory -- HIP event waits (stream-side or host-side) resolve against the newest signal of the other
    // stream at call time and would tie the stages together again (measured).  A call that yields no IF sample
    // decodes nothing and takes no slot.
    if (pipelined && N_if > 0) {
      pipe_seq++;
      k.par = (int)(pipe_seq % kPipe);
      // (one slot less than the ring holds: the slot of call N is still read at the head of call N+1, by the kernel that
      // carries its halos over, and that kernel is only ordered before the tail of call N+1)
      if (int rcw = wait_mark(&h_marks.p[1], pipe_seq > (unsigned long long)(kPipe - 1) ? pipe_seq - (kPipe - 1) : 0)) return rcw;
    }
    k.ifbuf = if_slot(k.par);
    last_if = k.ifbuf;
    dec_valid = !p.b_disc || env.debug_taps;   // the float copy of the discriminator output is a debug tap of the fused kernel
    if_valid = dec_valid;                  // ... and so are the IF samples behind its discriminator epilogue (the slot holds |x|^2 then)
    const long long top0 = (long long)rs.D * mA_prev + rs.ca() - p.prev.n_in;
    if (p.a == StageA::bank) {
      if (int rc = launch_chan(fes, k.d_iq, N_in, mA_prev, p.prev.n_in, count_mid)) return rc;
    } else if (p.a == StageA::decim16) {
      // R8B class, 10 MS/s: the matrix-core form behind the fused front end's input ring (runs: plan_call)
      using SH16 = Decim16Shape<10, 195>;
      FusedArgs a{};
      a.iq = k.d_iq; a.iq_stride = (long long)k.stride; a.n_valid = N_in;
      a.in_halo = d_in_halo.p; a.H_in = H_in; a.afragA = reinterpret_cast<const uint4 *>(d_dec16_afrag.p); a.hA = d_hA.p;
      a.zero16 = reinterpret_cast<const float2 *>(d_zero16.p);
      const long long lo0 = top0 - (rs.NA - 1);
      const int par16 = (int)(((lo0 % 2) + 2) % 2);
      a.nbase = lo0 - par16;
      a.count_mid = count_mid;
      a.mid = d_mid.p; a.mid_stride = (long long)(H_mid + max_mid); a.H_mid = H_mid;
      a.n_tiles = p.dec16_runs.tiles;
      a.tiles_per_wg = p.dec16_runs.tpw;
      const int grid16 = p.dec16_runs.grid;
      timed_on(fes, "ifr_decim", [&] {
        if (par16) hipLaunchKernelGGL((k_ifr_decim16<10, 195, 1>), dim3(grid16, S), dim3(DECIM16_THREADS), SH16::LDS_BYTES, fes, a);
        else hipLaunchKernelGGL((k_ifr_decim16<10, 195, 0>), dim3(grid16, S), dim3(DECIM16_THREADS), SH16::LDS_BYTES, fes, a);
      });
    } else if (p.a == StageA::decim2_16 || p.a == StageA::decim2_24) {
      const int s_pad = decim2_pad(qa);
      const size_t lds2 = sizeof(float2) * ((size_t)rs.D * s_pad + 2);   // + the spare slot
      const unsigned magic = (unsigned)((1u << 24) / (unsigned)rs.D + 1);
      const dim3 grid2((count_mid + kDecim2Out - 1) / kDecim2Out, S);
      timed_on(fes, "ifr_decim", [&] {
        auto go = [&](auto kern) {
          hipLaunchKernelGGL(kern, grid2, dim3(kDecim2Lanes), lds2, fes, k.d_iq, (long long)k.stride, N_in, d_in_halo.p, H_in,
                             d_hpA.p, rs.D, rs.ca(), top0 - rs.ca(), count_mid, d_mid.p,
                             (long long)(H_mid + max_mid), H_mid, (unsigned)(abs_in & 3u),
                             (int)cfg.enable_fourth_down, s_pad, magic);
        };
        constexpr int BL2 = kDecim2Lanes;
        const bool f4 = cfg.enable_fourth_down != 0;
        if (qa == 24) { f4 ? go(k_ifr_decim2<BL2, 24, 0, true>) : go(k_ifr_decim2<BL2, 24, 0, false>); return; }
        switch (in_fmt) {
        case 1: f4 ? go(k_ifr_decim2<BL2, 16, 0, true, 1, 1>) : go(k_ifr_decim2<BL2, 16, 0, false, 1, 1>); break;
        case 2: f4 ? go(k_ifr_decim2<BL2, 16, 0, true, 1, 2>) : go(k_ifr_decim2<BL2, 16, 0, false, 1, 2>); break;
        case 3: f4 ? go(k_ifr_decim2<BL2, 16, 0, true, 1, 3>) : go(k_ifr_decim2<BL2, 16, 0, false, 1, 3>); break;
        default: f4 ? go(k_ifr_decim2<BL2, 16, 0, true>) : go(k_ifr_decim2<BL2, 16, 0, false>); break;
        }
      });
    } else if (p.a == StageA::decim) {
      auto launch_decim = [&](auto bl_tag) {
        constexpr int BL = decltype(bl_tag)::value;
        const dim3 grid((count_mid + BL - 1) / BL, S);
        const size_t lds = sizeof(float2) * ((size_t)BL * rs.D + rs.NA - 1);
        hipLaunchKernelGGL(k_ifr_decim<BL>, grid, dim3(BL), lds, fes, k.d_iq, (long long)k.stride, N_in,
                           d_in_halo.p, H_in, d_hA.p, rs.NA, rs.D, top0, count_mid, d_mid.p,
                           (long long)(H_mid + max_mid), H_mid, (unsigned)(abs_in & 3u), cfg.enable_fourth_down);
      };
      const size_t per_out = sizeof(float2) * (size_t)rs.D, tail = sizeof(float2) * (size_t)(rs.NA - 1);
      timed_on(fes, "ifr_decim", [&] {
        if (256 * per_out + tail <= 60000) launch_decim(std::integral_constant<int, 256>{});
        else if (128 * per_out + tail <= 60000) launch_decim(std::integral_constant<int, 128>{});
        else launch_decim(std::integral_constant<int, 64>{});
      });
    }     // (fused: launched from run_tables)
    // stage B writes [if_off, if_off + N_if) of every row (every form stores only its own outputs): the chain's IF
    // buffer, or the caller's rows (front end only, fmr_resample_blocks_device)
    float2 *const ifbuf = if_out ? if_out : k.ifbuf;
    const long long mid_stride = H_mid + max_mid, if_stride = if_out ? if_out_stride : H_if + (long long)max_if;
    const int if_off = if_out ? 0 : H_if;
    if (if_out) if_valid = false;          // (nothing of this call in the IF buffer: fmr_debug_read 0 has no samples)
    if (p.b != StageB::none && !p.b_in_tables())
      timed_on(fes, "ifr_poly", [&] {
        // the tiled forms: tiles of 64 stage-B periods; the generic forms: 256 outputs per workgroup
        const long long P_first = kB_prev / rs.LB, P_last = (kB_prev + N_if - 1) / rs.LB;
        const int tiles = (int)((P_last - P_first) / 64 + 1);
        constexpr int BL = 256;
        const dim3 grid((unsigned)((N_if + BL - 1) / BL), S);
        const int span = (int)(((unsigned long long)(BL - 1) * rs.MB) / rs.LB) + rs.TB + 2;
        if (p.b == StageB::poly5h)
          hipLaunchKernelGGL((k_ifr_poly5h<48, 125>), dim3(std::min(tiles, n_cu), S), dim3(64 * FMR_POLY5H_WAVES), poly5h_lds,
                             fes, d_mid.p, mid_stride, mA_prev - H_mid, H_mid + count_mid, d_afrag5h.p,
                             poly5h_nkb, poly5h_inv_scale, rs.TB, kB_prev, (int)N_if, ifbuf, if_stride, if_off,
                             poly2_tile, tiles);
        else if (p.b == StageB::poly4_am) {
          const long long Pf = kB_prev / 48, Pl = (kB_prev + N_if - 1) / 48;
          const int tiles_am = (int)((Pl - Pf) / 64 + 1);
          hipLaunchKernelGGL((k_ifr_poly4<48, 128, 214>), dim3(std::min(tiles_am, 512), S), dim3(256),
                             sizeof(float2) * (size_t)(((poly4_am_tile + 127) / 128) * 128 + 4 * 8 * 48), fes, d_mid.p,
                             mid_stride, mA_prev - H_mid, H_mid + count_mid, d_afrag.p, kB_prev,
                             (int)N_if, ifbuf, if_stride, if_off, poly4_am_tile, tiles_am);
        } else if (p.b == StageB::poly4)
          hipLaunchKernelGGL((k_ifr_poly4<48, 125, 210>), dim3(std::min(tiles, 512), S), dim3(256),
                             sizeof(float2) * (size_t)(((poly2_tile + 127) / 128) * 128 + 4 * 8 * 48), fes, d_mid.p,
                             mid_stride, mA_prev - H_mid, H_mid + count_mid, d_afrag.p, kB_prev,
                             (int)N_if, ifbuf, if_stride, if_off, poly2_tile, tiles);
        else if (p.b == StageB::poly3)
          hipLaunchKernelGGL((k_ifr_poly3<384, 4>), dim3(tiles, S), dim3(384), sizeof(float2) * (size_t)poly2_tile, fes,
                             d_mid.p, mid_stride, mA_prev - H_mid, H_mid + count_mid, d_hBp.p, rs.TB,
                             (int)rs.LB, (int)rs.MB, d_bphi.p, d_boff.p, kB_prev, (int)N_if, ifbuf,
                             if_stride, if_off, poly2_tile);
        else if (p.b == StageB::poly2)
          hipLaunchKernelGGL(k_ifr_poly2<512>, dim3(tiles, S), dim3(512), sizeof(float2) * (size_t)poly2_tile, fes,
                             d_mid.p, mid_stride, mA_prev - H_mid, H_mid + count_mid, d_hB.p, rs.TB,
                             (int)rs.LB, (int)rs.MB, d_bphi.p, d_boff.p, kB_prev, (int)N_if, ifbuf,
                             if_stride, if_off, poly2_tile);
        else if (p.b == StageB::poly_frac) {
          // fractional-phase form: exact integer positions, call-relative on the device
          const __int128 tt = (__int128)kB_prev * rs.MB;
          const long long nk0 = (long long)(tt / rs.LB);
          const unsigned long long rem0 = (unsigned long long)(tt % rs.LB);
          hipLaunchKernelGGL(k_ifr_poly_frac<BL>, grid, dim3(BL), sizeof(float2) * (span + 4), fes, d_mid.p,
                             mid_stride, nk0 - rs.W() + 1 - (mA_prev - H_mid), H_mid + count_mid, d_hB.p,
                             rs.TB, hB_pitch, rs.LT, (unsigned long long)rs.LB, (unsigned long long)rs.MB, rem0, (int)N_if,
                             ifbuf, if_stride, if_off);
        } else
          hipLaunchKernelGGL(k_ifr_poly<BL>, grid, dim3(BL), sizeof(float2) * span, fes, d_mid.p,
                             mid_stride, mA_prev - H_mid, H_mid + count_mid, d_hB.p, rs.TB,
                             (unsigned)rs.LB, (unsigned)rs.MB, (unsigned long long)kB_prev * rs.MB, (int)N_if,
                             ifbuf, if_stride, if_off);
      });
    if (N_in > 0 && bank) {      // (one row; the pipelined R8B tail's k_fe_post leaves the input history to this kernel)
      timed_on(fes, "in_halo", [&] {
        hipLaunchKernelGGL((k_update_in_halo<256, 0>), dim3(1, 1), dim3(256), 0, fes, d_in_halo.p, H_in, k.d_iq, 0ll, N_in);
      });
    } else if (N_in > 0 && p.a != StageA::fused && !(p.b == StageB::poly5h_disc && pipelined)) {
      const long long stride = (long long)k.stride;
      timed_on(fes, "in_halo", [&] {
        switch (in_fmt) {
        case 1: hipLaunchKernelGGL((k_update_in_halo<256, 1>), dim3(1, S), dim3(256), 0, fes, d_in_halo.p, H_in, k.d_iq, stride, N_in); break;
        case 2: hipLaunchKernelGGL((k_update_in_halo<256, 2>), dim3(1, S), dim3(256), 0, fes, d_in_halo.p, H_in, k.d_iq, stride, N_in); break;
        case 3: hipLaunchKernelGGL((k_update_in_halo<256, 3>), dim3(1, S), dim3(256), 0, fes, d_in_halo.p, H_in, k.d_iq, stride, N_in); break;
        default: hipLaunchKernelGGL((k_update_in_halo<256, 0>), dim3(1, S), dim3(256), 0, fes, d_in_halo.p, H_in, k.d_iq, stride, N_in); break;
        }
      });
    }
  } else if (mpx_in) {      // (the PCM is read by mpxin_stage, behind the tables; there is no IF buffer)
    k.ifbuf = nullptr;
    last_if = nullptr;
    if_valid = gain_valid = false;
    dec_valid = true;
  } else {
    k.ifbuf = d_if.p;
    last_if = k.ifbuf;
    if_valid = true;
    if (N_if > 0)
      HIPCHK(hipMemcpy2DAsync(k.ifbuf + H_if, sizeof(float2) * (H_if + max_if), k.d_iq, sizeof(float2) * k.stride,
                              sizeof(float2) * N_if, S, hipMemcpyDeviceToDevice, stream));
  }
  abs_in += (unsigned long long)N_in;
  last_n_if = N_if; last_nb = k.nb; last_n_au = 0;
  k.ht = HaloTable{};
  if (has_rs && pipelined) {
    // the front-end stage keeps its own history: the stage-B halo is re-seated on its stream (after the fused kernel,
    // which is launched from run_tables, when that one runs)
    if (!p.b_in_tables()) {
      if (int rcf = finish_front_end_stage(k)) return rcf;
    }
  } else if (has_rs) {
    k.add_halo(d_mid.p, H_mid + (long long)max_mid, H_mid, count_mid);
  }
  if (!has_dec || N_if == 0) {
    hipLaunchKernelGGL(k_signal_host, dim3(1), dim3(1), 0, side, &h_marks.p[0], call_seq);   // no table this call
    if (k.audio_len) for (int b = 0; b < k.nb; b++) k.audio_len[b] = 0;
    if (has_dec && fir_enable && !pipelined) k.add_halo(k.ifbuf, H_if + (long long)max_if, H_if, N_if);
    if (k.ht.n) hipLaunchKernelGGL(k_shift_halo<256>, dim3(k.ht.n, S), dim3(256), 0, stream, k.ht);
    HIPCHK(hipGetLastError());
    k.done = true;                      // nothing to decode this call
  }
  return FMR_OK;
}

// Pipelined chain, end of the front-end stage on its stream: stage-B history for the next call, then the event the PLL
// stage of this call waits for.
int fmr_chain::finish_front_end_stage(CallCtx &k) {
  if (k.plan.count_mid > 0) {
    HaloTable hm{};
    hm.d[0] = HaloDesc{(unsigned *)d_mid.p, 2 * (H_mid + (long long)max_mid), 2 * H_mid, 2 * k.plan.count_mid};
    hm.n = 1;
    hipLaunchKernelGGL(k_shift_halo<256>, dim3(1, S), dim3(256), 0, stream, hm);
  }
  if (has_dec && k.N_if > 0) {
    HIPCHK(hipEventRecord(ev_fe[k.par], stream));
    // the previous call's tail stage: behind this front end, beside this call's PLL stage
    if (int rc = flush_tail(ev_fe[k.par])) return rc;
  }
  return FMR_OK;
}

// First block of every workgroup's run of a tiled front-end kernel (the epilogue walks the block table from there): the
// block that holds the run's first IF sample, kb_ref + tile_len x its first tile -- tile0[w] when given (the fused front
// end's runs of equal weight), else balanced runs of r.tpw tiles, the first r.rem of them one tile longer
void fmr_chain::fill_run_blocks(const CallCtx &k, int *blk0, const TileRuns &r, const int *tile0, long long kb_ref, int tile_len) {
  int b = 0;
  for (int w = 0; w < r.grid; w++) {
    const long long t = tile0 ? tile0[w] : (long long)w * r.tpw + std::min(w, r.rem);
    const long long kf = std::max<long long>(0, kb_ref + tile_len * t);
    while (b < k.nb && (long long)k.tab.if_off[b] + k.tab.if_len[b] <= kf) b++;
    blk0[w] = b;
  }
}

// per-call block / chunk tables on the side stream, then the fused front end (it needs the block table)
int fmr_chain::run_tables(CallCtx &k) {
  const CallPlan &p = k.plan;
  const int nb = k.nb;
  const long long N_if = k.N_if;
  int *const h_tab = k.h_tab, *const d_tab_slot = k.d_tab_slot;
  // --------------------------------------------------------------- block tables
  k.N_au = 0;
  k.any_mpf = false;
  k.amA_prev = arsc.mA; k.akB_prev = arsc.kB; k.an_prev = arsc.n_in;
  for (int b = 0; b < nb; b++) {
    k.tab.mpf[b] = 0;
    k.tab.au_off[b] = (int)k.N_au;
    k.tab.au_len[b] = 0;
    if (k.tab.if_len[b] == 0) continue;          // the decoder is not called for an empty IF block (main.cpp:931-934)
    if (mode == FMR_MODE_FM) {
      if (wait_multipath_blocks > 0) wait_multipath_blocks--;     // FmDecode.cpp:107-110
      else if (enable_mpf) { k.tab.mpf[b] = 1; k.any_mpf = true; }
      const long long n = arsc.advance(ars, k.tab.if_len[b]);
      k.tab.au_len[b] = (int)n;
      k.N_au += n;
    } else {
      k.tab.au_len[b] = k.tab.if_len[b];
      k.N_au += k.tab.if_len[b];
    }
  }
  last_n_au = k.N_au;
  // PLL chunk table: every decoder block is cut into chunks of <= C_PLL samples
  // The per-chunk arrays (off, len, blk) are filled on the device from the block table; the
  // host only sends 6*max_blocks+1 ints per call.
  int *t_first = h_tab + 5 * (size_t)max_blocks;
  k.nck = 0;
  for (int b = 0; b < nb; b++) {
    t_first[b] = k.nck;
    k.nck += (k.tab.if_len[b] + p.c_call - 1) / p.c_call;
  }
  t_first[nb] = k.nck;
  const size_t head_ints = 6 * (size_t)max_blocks + 1;
  // a kernel pulls the table out of the pinned host slot: hipMemcpyAsync H2D made the caller wait for the
  // stream to drain up to the copy (0.5-1 ms of host time per call), a launch does not
  // Table kernels and the PLL's initial node guess run on the side stream, beside the front end.
  hipLaunchKernelGGL(k_copy_ints, dim3((unsigned)((head_ints + 255) / 256)), dim3(256), 0, side,
                     (const int *)h_tab, d_tab_slot, (int)head_ints);
  // the table's tail: first block (fused front end: and first macro tile) of every run of the front end's tiled kernel,
  // first block of every run of the IF filter's
  int *const t_wg = h_tab + (tab_ints - kMaxFusedWg), *const d_wg = d_tab_slot + (tab_ints - kMaxFusedWg);
  // the kernel's own tables: first block of every workgroup and, when the front end runs a call ahead of the decoder,
  // the block table too (the side stream's copy of it sits behind the previous call's lock logic; both copies write
  // the same values)
  auto copy_runs = [&](int n) {
    if (pipelined)
      hipLaunchKernelGGL(k_copy_ints2, dim3((unsigned)((n + 2 * (size_t)max_blocks + 255) / 256)), dim3(256), 0, stream,
                         (const int *)t_wg, d_wg, n, (const int *)h_tab, d_tab_slot, 2 * max_blocks);
    else
      hipLaunchKernelGGL(k_copy_ints, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, side, (const int *)t_wg, d_wg, n);
  };
  const TileRuns &fr = p.fe_runs;
  k.fused_n_tiles = 0; k.fused_kb_ref = 0;
  const long long fused_T_first = p.prev.kB / 48 / 8;
  if (p.b == StageB::fused) {
    // one workgroup per CU: contiguous runs of macro tiles, the streams share the CUs
    k.fused_n_tiles = fr.tiles;
    fe_spare_cus = std::max(0, n_cu - fr.grid * S);
    const long long kb_ref = 384 * fused_T_first - p.prev.kB;
    // Where the runs start: a macro tile whose epilogue writes the per-block partial sums (the last ~400 blocks of a call:
    // block walk, six wave reductions and a store per 128 samples) costs its workgroup kFusedSumWeight more than one that does
    // not -- measured, round 6: the workgroups of the last fifth of a 2048-block call took 207-213 us against the others' 194-197
    // and the launch ended with them (with weight 0.05 they still did, with 0.11 the last to end are spread over the chip).  Runs of equal WEIGHT instead of equal length; the table's tail carries the first tile of
    // every run behind the first block of every run.
    int *t_tile0 = t_wg + kFusedTile0Off;
    {
      const double eps = p.b_disc ? (env.x_sumw >= 0 ? env.x_sumw * 1e-3 : kFusedSumWeight) : 0.0;
      const long long tp = std::min<long long>(fr.tiles, std::max<long long>(0, (p.part_from - kb_ref) / 384));   // first tile with sums
      const double W = (double)tp + (double)(fr.tiles - tp) * (1.0 + eps);
      t_tile0[0] = 0;
      for (int w = 1; w < fr.grid; w++) {
        const double cum = W * w / fr.grid;
        const double tt = cum <= (double)tp ? cum : (double)tp + (cum - (double)tp) / (1.0 + eps);
        int ti = (int)(tt + 0.5);
        ti = std::max(ti, t_tile0[w - 1] + 1);                              // every run holds a tile
        ti = std::min(ti, fr.tiles - (fr.grid - w));                        // ... the later ones too
        t_tile0[w] = ti;
      }
      t_tile0[fr.grid] = fr.tiles;
    }
    fill_run_blocks(k, t_wg, fr, t_tile0, kb_ref, 384);
    copy_runs(kFusedTile0Off + fr.grid + 1);
  }
  const TileRuns &ir = p.fir_runs;
  if (p.fir_tail()) {
    fill_run_blocks(k, t_wg + kFirBlk0Off, ir, nullptr, 0, 3072);
    hipLaunchKernelGGL(k_copy_ints, dim3((unsigned)((ir.grid + 255) / 256)), dim3(256), 0, side,
                       (const int *)(t_wg + kFirBlk0Off), d_wg + kFirBlk0Off, ir.grid);
  }
  if (p.b == StageB::poly5h_disc) {
    // R8B class: the table's tail carries the block that holds the first IF sample of every run, as for the fused front end
    k.fused_n_tiles = 8 * fr.tiles;                             // in the epilogue's macro tiles of 384 samples
    const long long kb_ref = 48 * (p.prev.kB / 48) - p.prev.kB;
    k.fused_kb_ref = (int)kb_ref;
    fill_run_blocks(k, t_wg, fr, nullptr, kb_ref, 3072);
    copy_runs(fr.grid);
  }
  int *d_first = d_tab_slot + 5 * (size_t)max_blocks;
  int *d_ck = d_tab_slot + head_ints;
  k.ct = ChunkTab{d_ck, d_ck + max_ck, d_ck + 2 * max_ck, d_first, k.nck};
  hipLaunchKernelGGL(k_signal_host, dim3(1), dim3(1), 0, side, &h_marks.p[0], call_seq);
  if (mode == FMR_MODE_FM && k.nck > 0) {
    hipLaunchKernelGGL(k_chunk_tab, dim3(nb), dim3(64), 0, side, d_tab_slot, d_tab_slot + max_blocks, d_first, p.c_call,
                       d_ck, d_ck + max_ck, d_ck + 2 * max_ck);
    if (stereo && !env.serial)
      timed_on(side, "pll_begin", [&] {
        hipLaunchKernelGGL(k_pll_begin, dim3((k.nck + 1 + 63) / 64, S), dim3(64), 0, side, d_pll_nodes.p, k.ct, d_state.p,
                           pllc);
      });
  }
  // FM without the equaliser: the round flags and the AGC's start nodes are reset here too, beside the front end (5-10 us
  // of the critical path when launched between the front end and the PLL's first pass).  Their last readers of the previous
  // call are the PLL kernels (ordered before this stream's k_pll_finish) and the side-stream AGC (ev_agc).
  if (p.iter_on_side) {
    if (ev_agc_live) HIPCHK(hipStreamWaitEvent(side, ev_agc, 0));
    hipLaunchKernelGGL(k_iter_begin, dim3(S), dim3(256), 0, side, d_flags.p, d_agc_nodes.p, p.agc_nc, d_state.p, S,
                       (unsigned long long *)d_pll_sync.p, (int)(sizeof(PllSync) / 8), d_pll_tick2.p, pll_tick2_per_stream, d_agc_tick.p);
  }
  if (pipelined && ring_prev >= 0 && ring_prev != k.par) {
    // halos of this call's ring slot = the tail of the previous call's slot (its writers -- front end, discriminator, PLL
    // -- are ordered before this stream's lock logic of that call; nothing of this call touches the head of a slot)
    CarryTable ctab{};
    const long long bstr = H_b + (long long)max_if;
    const int np = (int)ring_prev_n;
    ctab.d[ctab.n++] = CarryDesc{(const unsigned *)base_slot(ring_prev), (unsigned *)k.base, bstr, H_b, np};
    if (stereo) ctab.d[ctab.n++] = CarryDesc{(const unsigned *)raw_slot(ring_prev), (unsigned *)k.raw, 2 * bstr, 2 * H_b, 2 * np};
    if (fir_enable) ctab.d[ctab.n++] = CarryDesc{(const unsigned *)if_slot(ring_prev), (unsigned *)k.ifbuf, 2 * (H_if + (long long)max_if), 2 * H_if, 2 * np};
    hipLaunchKernelGGL(k_carry_halo<256>, dim3(ctab.n, S), dim3(256), 0, side, ctab);
  }
  // the decoder waits for the tables.  In the pipelined chain the front end shares its stream and must not: the wait is
  // enqueued behind the front end's launch (below)
  HIPCHK(hipEventRecord(ev_tab, side));
  if (!pipelined) HIPCHK(hipStreamWaitEvent(stream, ev_tab, 0));
  k.bt = BlockTab{d_tab_slot, d_tab_slot + max_blocks, d_tab_slot + 2 * max_blocks, d_tab_slot + 3 * max_blocks,
                  d_tab_slot + 4 * max_blocks, nb};
  k.if_stride = H_if + (long long)max_if;
  // the discriminator's carried phase: when the previous call ran the discriminator in its decoder stage (a call too
  // short for the fused kernel), its phase is committed by that call's statistics kernel on the side stream
  if (pipelined && p.b_disc && disc_commit_on_side) HIPCHK(hipStreamWaitEvent(stream, ev_stats, 0));
  if (p.b == StageB::fused) {
    // ---- fused front end: needs the block table (per-block statistics), hence launched here, after the table copy
    constexpr int D = kFusedD, NA = kFusedNA;
    FusedArgs a{};
    a.iq = k.d_iq; a.iq_stride = (long long)k.stride; a.n_valid = k.N_in;
    a.in_halo = d_in_halo.p; a.H_in = H_in; a.afragA = reinterpret_cast<const uint4 *>(d_fused_afragA.p); a.hA = d_hA.p; a.hB = d_hB.p;
    const long long n0 = (long long)rs.D * p.prev.mA - p.prev.n_in;
    const long long lo0 = n0 + rs.ca() - (NA - 1);
    const int par = (int)(((lo0 % 2) + 2) % 2);
    a.nbase = lo0 - par;
    constexpr int kME = FusedShape<kFusedD, kFusedNA>::ME, kEPT = FusedShape<kFusedD, kFusedNA>::EPT;
    const long long T_first = fused_T_first, E_ref = kEPT * T_first - 1;
    a.j_ref = (int)(kME * E_ref + 104 - p.prev.mA);
    a.pos_ref = (int)((((kME * E_ref + 208) % 3000) + 3000) % 3000);
    a.t3_ref = (int)(T_first % 3);
    a.kb_ref = (int)(384 * T_first - p.prev.kB);
    a.count_mid = p.count_mid;
    a.mid = d_mid.p; a.mid_stride = (long long)(H_mid + max_mid); a.H_mid = H_mid;
    a.afragB = reinterpret_cast<const uint4 *>(d_fused_afragB.p); a.hB_inv_scale = fused_hB_inv_scale; a.n_if = (int)N_if;
    a.out = k.ifbuf; a.out_stride = k.if_stride; a.out_off = H_if;
    k.nrm = nullptr;
    if (p.b_disc && !env.debug_taps) {
      // nobody but the AGC's state solve reads the IF behind the discriminator epilogue: it gets |x|^2 (4 B per sample, in the
      // IF slot's memory) and the IF samples stay on chip
      a.out = nullptr;
      a.nrm = reinterpret_cast<float *>(k.ifbuf); a.nrm_stride = 2 * k.if_stride; a.nrm_off = 0;
      k.nrm = a.nrm; k.nrm_stride = a.nrm_stride;
    }
    a.n_tiles = fr.tiles;
    a.tiles_per_wg = fr.tpw;
    const int grid = fr.grid;
    a.wg_blk0 = d_wg;
    a.wg_tile0 = a.wg_blk0 + kFusedTile0Off;
    a.zero16 = reinterpret_cast<const float2 *>(d_zero16.p);
    a.base = p.b_disc ? k.base : nullptr;        // null: IF samples only (an IF FIR or the equaliser comes first)
    a.base_stride = H_b + (long long)max_if; a.base_off = H_b;
    a.dec = env.debug_taps ? d_dec.p : nullptr; a.dec_stride = (long long)max_if;
    a.nf = disc_nf; a.bound = disc_bound;
    a.st = d_state.p; a.hB_last = d_hB_last.p; a.part = k.part;
    a.if_off = k.bt.if_off; a.if_len = k.bt.if_len; a.nb = nb;
    a.part_from = p.part_from;
    constexpr size_t kLds = FusedShape<D, NA>::LDS_BYTES;
    hipStream_t fes = stream;
    if (d_fe_stamps.p) { a.stamps = d_fe_stamps.p; fe_stamps_n = grid * S; }
    a.mid32 = d_fused_mid32.p;
    if (d_fe_stamps.p) hipLaunchKernelGGL(k_fused_stamp, dim3(1), dim3(1), 0, fes, stamp_slot(0), 16 * kStampCalls);
    timed_on(fes, "ifr_fused", [&] {
      if (ext_a) {      // (timed with the events of its own dispatch)
        if (par) hipExtLaunchKernelGGL((k_ifr_fused<D, NA, 1, 0>), dim3(grid, S), dim3(FUSED_THREADS), kLds, fes, ext_a, ext_b, 0, a);
        else hipExtLaunchKernelGGL((k_ifr_fused<D, NA, 0, 0>), dim3(grid, S), dim3(FUSED_THREADS), kLds, fes, ext_a, ext_b, 0, a);
        return;
      }
      if (par) hipLaunchKernelGGL((k_ifr_fused<D, NA, 1, 0>), dim3(grid, S), dim3(FUSED_THREADS), kLds, fes, a);
      else hipLaunchKernelGGL((k_ifr_fused<D, NA, 0, 0>), dim3(grid, S), dim3(FUSED_THREADS), kLds, fes, a);
    });
    if (d_fe_stamps.p) hipLaunchKernelGGL(k_fused_stamp, dim3(1), dim3(1), 0, fes, stamp_slot(1), 0);
    k.fused_kb_ref = a.kb_ref;
  }
  if (p.b == StageB::poly5h_disc) {
    // ---- R8B class: stage B with the discriminator epilogue (the fused front end's, a wave per 384 staged samples)
    FusedArgs a{};
    a.n_if = (int)N_if; a.kb_ref = k.fused_kb_ref;
    a.out = nullptr; a.out_stride = k.if_stride; a.out_off = H_if;
    a.nrm = reinterpret_cast<float *>(k.ifbuf); a.nrm_stride = 2 * k.if_stride; a.nrm_off = 0;
    if (env.debug_taps) { a.out = k.ifbuf; a.nrm = nullptr; }      // the IF samples themselves (fmr_debug_read 0); the AGC reads them then
    k.nrm = a.nrm; k.nrm_stride = a.nrm_stride;
    a.base = k.base; a.base_stride = H_b + (long long)max_if; a.base_off = H_b;
    a.dec = env.debug_taps ? d_dec.p : nullptr; a.dec_stride = (long long)max_if;
    a.nf = disc_nf; a.bound = disc_bound;
    a.st = d_state.p; a.part = k.part; a.n_tiles = k.fused_n_tiles; a.part_from = p.part_from;
    a.if_off = k.bt.if_off; a.if_len = k.bt.if_len; a.nb = nb;
    a.wg_blk0 = d_wg;
    a.mid32 = d_run_ph.p;
    timed_on(stream, "ifr_poly", [&] {
      hipLaunchKernelGGL((k_ifr_poly5h<48, 125, Poly5hDiscEpi>), dim3(fr.grid, S), dim3(64 * FMR_POLY5H_WAVES), poly5h_lds, stream,
                         d_mid.p, (long long)(H_mid + max_mid), p.prev.mA - H_mid, H_mid + p.count_mid, d_afrag5h.p,
                         poly5h_nkb, poly5h_inv_scale, rs.TB, p.prev.kB, (int)N_if, (float2 *)nullptr, 0ll, 0, poly2_tile, fr.tiles,
                         a, fr.tpw, fr.rem);
      if (fr.grid > 1)
        hipLaunchKernelGGL(k_poly5h_heads, dim3((fr.grid + 62) / 64, S), dim3(64), 0, stream, a, fr.grid, fr.tpw, fr.rem);
    });
  }
  if (pipelined && p.b_in_tables()) {
    // The PLL stage starts from here.  What the front-end stage carries into its next call -- the input history (a bank's
    // is left to its own kernel), the stage-B history, the discriminator's last phase -- is one small kernel on its stream;
    // when that stream is the decoder's it is launched behind the PLL's first pass (run_fm_pll), not between the front end
    // and that pass.
    HIPCHK(hipEventRecord(ev_fe[k.par], stream));
    k.fe_post = FePostJob{k.d_iq, (long long)k.stride, bank ? 0ll : k.N_in, p.count_mid, (int)p.b_disc, true};
    // the previous call's tail stage: behind this front end, beside this call's PLL stage
#ifndef FMR_FIR_TAIL_EARLY
    // (... and behind the IF filter's kernel where that one sits between front end and PLL: run_fm)
    if (p.fir_tail()) { k.tail_deferred = true; if (int rc = flush_walk()) return rc; } else
#endif
    if (int rc = flush_tail(ev_fe[k.par])) return rc;
  }
  if (pipelined) HIPCHK(hipStreamWaitEvent(stream, ev_tab, 0));
  return FMR_OK;
}

// Pipelined chain: what the front-end stage carries into its next call (input history, stage-B history, the discriminator's
// last phase), one small kernel on the decoder stream, if this call still owes it.
void fmr_chain::launch_fe_post(FePostJob &j) {
  if (!j.pending) return;
  j.pending = false;
  hipLaunchKernelGGL(k_fe_post<256>, dim3(3, S), dim3(256), 0, stream, d_in_halo.p, H_in, j.d_iq, j.stride, j.n_in,
                     d_mid.p, (long long)(H_mid + max_mid), H_mid, j.count_mid, d_state.p, j.commit);
}

// IF-rate part common to all decoders: fine tuner, IF filter + level, IF AGC
int fmr_chain::run_if_stage(CallCtx &k) {
  const CallPlan &p = k.plan;
  const int nb = k.nb;
  const long long N_if = k.N_if, if_stride = k.if_stride;
  float2 *const ifbuf = k.ifbuf; const BlockTab &bt = k.bt;
  // ------------------------------------------------------- decoder, IF-rate part
  // SSB / WSPR: mix the new IF samples in place before the filter (the filter history in the halo is already mixed)
  if (ssb_like && d_ft_pre.p)
    timed("finetune_pre", [&] {
      hipLaunchKernelGGL(k_finetune<256>, dim3(nb, S), dim3(256), 0, stream, ifbuf, if_stride, H_if, bt, d_ft_pre.p,
                         480, ft_index, (float *)nullptr);
    });
  if (p.fir == IfForm::poly4_disc) {
    FusedArgs a{};
    a.n_if = (int)N_if; a.kb_ref = 0;
    a.out = d_fir.p; a.out_stride = (long long)max_if; a.out_off = 0;
    a.base = k.base; a.base_stride = H_b + (long long)max_if; a.base_off = H_b;
    a.dec = env.debug_taps ? d_dec.p : nullptr; a.dec_stride = (long long)max_if;
    a.nf = disc_nf; a.bound = disc_bound;
    const TileRuns &r = p.fir_runs;
    a.st = d_state.p; a.part = k.part; a.n_tiles = 8 * r.tiles; a.part_from = p.part_from;
    a.if_off = bt.if_off; a.if_len = bt.if_len; a.nb = nb;
    a.wg_blk0 = k.d_tab_slot + (tab_ints - kMaxFusedWg) + kFirBlk0Off;
    a.mid32 = d_run_ph.p;
    a.fir_c0 = h_coeff0; a.fir_order = ntaps - 1; a.hA = d_coeff.p;      // (hA: the filter's taps, for the repair of tiles that hold a non-finite sample)
    timed("fm_block", [&] {
      constexpr int kTile = 64 * 48 + 47 + 127 + 64;
      hipLaunchKernelGGL((k_ifr_poly4<48, 48, 127, 2, Poly4FirDiscEpi>), dim3(r.grid, S), dim3(256),
                         sizeof(float2) * (size_t)(((kTile + 127) / 128) * 128 + 4 * 8 * 48), stream, ifbuf, if_stride,
                         (long long)(64 - H_if), H_if + (int)N_if, d_afrag_fir_fm.p, 0ll, (int)N_if, (float2 *)nullptr, 0ll, 0,
                         kTile, r.tiles, a, r.tpw, r.rem);
      if (r.grid > 1)
        hipLaunchKernelGGL(k_poly5h_heads, dim3((r.grid + 62) / 64, S), dim3(64), 0, stream, a, r.grid, r.tpw, r.rem);
    });
  } else if (p.fir != IfForm::none) {
    timed("fm_block", [&] {
      // four outputs per lane; FM without the equaliser: the discriminator is its epilogue (k_disc is not launched)
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(nb, S), dim3(256), p.lds_fb, stream, ifbuf, if_stride, H_if, bt,
                           d_coeff.p, ntaps, (int)(mode != FMR_MODE_FM), d_fir.p, (long long)max_if, d_if_rms_blk.p,
                           disc_nf, disc_bound, d_dec.p, (long long)max_if, k.base, H_b + (long long)max_if, H_b,
                           d_bb_mean_blk.p, d_bb_rms_blk.p, d_blk_ph.p, p.TL);
      };
      if (p.fir == IfForm::block3_disc) {
        go(k_fm_block3<256, true>);
        hipLaunchKernelGGL(k_disc_heads, dim3((nb + 255) / 256, S), dim3(256), 0, stream, bt, d_blk_ph.p, disc_bound, d_dec.p,
                           (long long)max_if, k.base, H_b + (long long)max_if, H_b, d_bb_mean_blk.p, d_bb_rms_blk.p, d_state.p);
      } else if (p.fir == IfForm::block3) go(k_fm_block3<256, false>);       // (FM with the equaliser behind the filter)
      else if (p.fir == IfForm::poly4_finish) {
        // AM / DSB / NBFM, 255 or 127 taps: the matrix-core form (call-relative periods of 48 outputs; buffer index m of the
        // kernel's window arithmetic is x[m - (order - (W - 1))], W = taps / 2: the "absolute" index of the buffer's first element
        // is order - W + 1 - H_if)
        const int order = ntaps - 1, Wf = ntaps >> 1;
        const int kTile = 64 * 48 + 47 + ntaps + 64;
        const int tiles_f = (int)((N_if - 1) / 48 / 64 + 1);
        auto gof = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3(std::min(tiles_f, 1024), S), dim3(256),
                             sizeof(float2) * (size_t)(((kTile + 127) / 128) * 128 + 4 * 8 * 48), stream, ifbuf, if_stride,
                             (long long)(order - Wf + 1 - H_if), H_if + (int)N_if, d_afrag_fir.p, 0ll, (int)N_if, d_fir.p, (long long)max_if, 0,
                             kTile, tiles_f, Poly5hStoreIf::Args{}, 0, 0);
        };
        if (ntaps == 255) gof(k_ifr_poly4<48, 48, 255, 1>); else gof(k_ifr_poly4<48, 48, 127, 2>);
        hipLaunchKernelGGL(k_fir_finish<256>, dim3(nb, S), dim3(256), 0, stream, ifbuf, if_stride, H_if, bt, d_coeff.p, ntaps,
                           d_fir.p, (long long)max_if, d_if_rms_blk.p);
      } else if (p.fir == IfForm::block2) {
        // the 48 kHz modes: blocks of a few hundred samples behind 255 or 2049 taps, nearly every output a head output
        constexpr int TL2 = 1024;
        const size_t lds2 = sizeof(float2) * ((size_t)(ntaps - 1) + TL2) + sizeof(float) * (size_t)ntaps;
        hipLaunchKernelGGL((k_fm_block2<256, TL2>), dim3(nb, S), dim3(256), lds2, stream, ifbuf, if_stride, H_if, bt,
                           d_coeff.p, ntaps, (int)(mode != FMR_MODE_FM), d_fir.p, (long long)max_if, d_if_rms_blk.p);
      } else
        hipLaunchKernelGGL(k_fm_block<256>, dim3(nb, S), dim3(256), 0, stream, ifbuf, if_stride, H_if, bt, d_coeff.p,
                           ntaps, (int)fir_enable, (int)(mode != FMR_MODE_FM), d_fir.p, (long long)max_if,
                           d_if_rms_blk.p);
    });
  }
  if (ssb_like) {    // mix the filter output in place; the IF level is measured after it (AmDecode.cpp:114,122,128,136,154)
    timed("finetune_post", [&] {
      hipLaunchKernelGGL(k_finetune<256>, dim3(nb, S), dim3(256), 0, stream, d_fir.p, (long long)max_if, 0, bt,
                         d_ft_post.p, 480, ft_index, d_if_rms_blk.p);
    });
    ft_index = (unsigned)((ft_index + (unsigned long long)N_if) % 480u);
  }
  k.xin = fir_enable ? d_fir.p : ifbuf;
  k.x_stride = fir_enable ? (long long)max_if : if_stride;
  k.x_off = fir_enable ? 0 : H_if;
  // ---- IF AGC: Newton multiple shooting over chunks of C_AGC samples (kernels_par.hpp)
  k.disc_gain = d_gain.p;      // gain sequence the discriminator multiplies in (nullptr = none)
  k.agc_on_side = false; k.agc_deferred = false; agc_beside_mpf = false;
  if (!p.iter_on_side)
    hipLaunchKernelGGL(k_iter_begin, dim3(S), dim3(256), 0, stream, d_flags.p,
                       (env.serial || enable_mpf) ? (float *)nullptr : d_agc_nodes.p,
                       p.agc_nc, d_state.p, S, (unsigned long long *)d_pll_sync.p, (int)(sizeof(PllSync) / 8), d_pll_tick2.p,
                       pll_tick2_per_stream, d_agc_tick.p);
  switch (p.agc) {
  case AgcPlace::beside_mpf:
    // With the equaliser on, the AGC'd amplitude feeds the constant-modulus error, and the equaliser kernel is the serial
    // bottleneck anyway: the exact serial AGC, beside the equaliser, which consumes the gains as they are published
    // (k_if_agc_wave / k_mpf4, kernels.hpp).  The progress words count the samples of THIS call: zeroed here, in front of both
    // kernels -- a call that failed half way cannot leave a count behind that a later call would take for its own.
    HIPCHK(hipMemsetAsync(d_agc_progress.p, 0, sizeof(unsigned long long) * (size_t)S, stream));
    HIPCHK(hipEventRecord(ev_if, stream));
    HIPCHK(hipStreamWaitEvent(side2, ev_if, 0));
#ifdef FMR_AB_PARTNERS
    if (env.test_agc_late > 0)      // test hook: the AGC kernel starts this many milliseconds late
      hipLaunchKernelGGL(k_hold_stream, dim3(1), dim3(1), 0, side2, (unsigned long long)env.test_agc_late * 100000ull);
#endif
    timed_on(side2, "if_agc", [&] {
      if (env.test_agc_late >= 0)   // (test hook, < 0: the AGC kernel is not launched at all)
      hipLaunchKernelGGL(k_if_agc_wave, dim3(S), dim3(64), 0, side2, k.xin, k.x_stride, k.x_off, (int)N_if, d_gain.p,
                         (long long)max_if, d_state.p, agc_init, agc_max, agc_rate, d_agc_progress.p);
    });
    HIPCHK(hipEventRecord(ev_agc, side2));
    ev_agc_live = agc_beside_mpf = true;
    break;
  case AgcPlace::serial:
    timed("if_agc", [&] {
      hipLaunchKernelGGL(k_if_agc, dim3((S + 63) / 64), dim3(64), 0, stream, k.xin, k.x_stride, k.x_off, (int)N_if, d_gain.p,
                         (long long)max_if, d_state.p, S, agc_init, agc_max, agc_rate, (unsigned long long *)nullptr);
    });
    break;
  case AgcPlace::aside_after_pll: case AgcPlace::aside: case AgcPlace::in_line: {
    // FM without the equaliser (aside): the AGC output only feeds atan2, which is invariant to the (positive) gain, so the
    // discriminator reads the un-gained samples and the gain recurrence -- still solved exactly as before, its state carries
    // -- runs on the side stream, off the critical path (the two paths differ by 3.8e-8 RMS of float rounding).
    AgcJob &j = k.agc;
    j.aside = p.agc != AgcPlace::in_line;
    j.xin = k.xin; j.x_stride = k.x_stride; j.x_off = k.x_off;
    j.nrm_in = (j.aside && !fir_enable) ? k.nrm : nullptr; j.nrm_stride = k.nrm_stride;
    j.N_if = N_if; j.nc = p.agc_nc; j.iters = p.agc_iters;
    // the discriminator does not see the gains then -- the recurrence is solved for its state only, and its 4 bytes per IF
    // sample stay out of HBM unless the debug tap asks for them
    j.gain_out = (j.aside && !env.debug_taps) ? (float *)nullptr : d_gain.p;
    j.ginv = (mode == FMR_MODE_FM || mode == FMR_MODE_NBFM) ? (j.gain_out ? 1 : 2) : -env.x_amtol;
    if (j.aside) { k.disc_gain = nullptr; k.agc_on_side = true; }
    gain_valid = j.gain_out != nullptr;
    // With the PLL on, the side-stream AGC starts only after the PLL's first (Jacobian) integration pass: that
    // pass runs one wave per SIMD and every co-resident AGC wave stretches it (measured 118 -> 160 us).
    k.agc_deferred = p.agc == AgcPlace::aside_after_pll;
    if (!k.agc_deferred) { if (int rca = enqueue_agc(j, nullptr)) return rca; }
    break;
  }
  }
  return FMR_OK;
}

// The IF AGC's Newton rounds and their fallback, on side2 behind `gate` (null: behind a new marker on the decoder stream)
// when the job runs aside, else on the decoder stream.
int fmr_chain::enqueue_agc(const AgcJob &j, hipEvent_t gate) {
  hipStream_t as = j.aside ? side2 : stream;
  if (j.aside && !gate) { HIPCHK(hipEventRecord(ev_if, stream)); gate = ev_if; }
  if (j.aside) HIPCHK(hipStreamWaitEvent(side2, gate, 0));
  timed_on(as, "if_agc", [&] {
    // (four waves, one per SIMD: a workgroup of sixteen finds no compute unit with room for all of them while the PLL's
    // first pass -- one 260-register wave per SIMD, 1258 workgroups queueing -- holds the chip)
    constexpr int kAgcWg = 256;
    const size_t agc_ballast = j.aside ? side_ballast() : 0;
    const dim3 rgrid((j.nc + kAgcWg - 1) / kAgcWg, S);
    for (int it = 0; it < j.iters; it++) {
      if (j.nrm_in)
        hipLaunchKernelGGL((k_agc_round<C_AGC, float>), rgrid, dim3(kAgcWg), agc_ballast, as, j.nrm_in, j.nrm_stride, 0, (int)j.N_if,
                           j.gain_out, (long long)max_if, d_agc_nodes.p, d_agc_G.p, d_agc_M.p, j.nc, agc_init, agc_max,
                           agc_rate, d_state.p, d_flags.p, j.ginv, d_agc_tick.p);
      else
        hipLaunchKernelGGL((k_agc_round<C_AGC, float2>), rgrid, dim3(kAgcWg), agc_ballast, as, j.xin, j.x_stride, j.x_off, (int)j.N_if,
                           j.gain_out, (long long)max_if, d_agc_nodes.p, d_agc_G.p, d_agc_M.p, j.nc, agc_init, agc_max,
                           agc_rate, d_state.p, d_flags.p, j.ginv, d_agc_tick.p);
    }
    if (j.nrm_in)
      hipLaunchKernelGGL(k_if_agc_fallback<float>, dim3((S + 63) / 64), dim3(64), 0, as, j.nrm_in, j.nrm_stride, 0, (int)j.N_if,
                         j.gain_out, (long long)max_if, d_state.p, S, agc_init, agc_max, agc_rate, d_flags.p);
    else
      hipLaunchKernelGGL(k_if_agc_fallback<float2>, dim3((S + 63) / 64), dim3(64), 0, as, j.xin, j.x_stride, j.x_off, (int)j.N_if,
                         j.gain_out, (long long)max_if, d_state.p, S, agc_init, agc_max, agc_rate, d_flags.p);
  });
  if (j.aside) { HIPCHK(hipEventRecord(ev_agc, side2)); ev_agc_live = true; }
  return FMR_OK;
}

// PilotPhaseLock: Newton multiple shooting over chunks (kernels_par.hpp); beside it, on side2, the IF AGC and the mono
// audio tail; after it, on side, the lock logic.  Says in t which of these the tail has to wait for.
int fmr_chain::run_fm_pll(CallCtx &k, TailCtx &t) {
  const CallPlan &p = k.plan;
  const int nb = k.nb, nck = k.nck;
  const ChunkTab &ct = k.ct; const BlockTab &bt = k.bt;
  const long long base_stride = H_b + (long long)max_if;
  const bool split_mono = t.can_split && !pipelined;      // the mono channel of the audio tail beside the PLL, on side2
  if (env.serial) {
    timed("pll", [&] {
      hipLaunchKernelGGL(k_pll, dim3((S + 63) / 64), dim3(64), 0, stream, k.base, base_stride, H_b, bt, k.raw,
                         base_stride, H_b, d_atan.p, pllc, (int)pilot_shift, k.stereo_blk, d_state.p, S);
    });
  } else {
    // ---- pilot PLL: Newton multiple shooting over chunks of C_PLL samples
    int rc_agc = FMR_OK;          // a failure inside the lambda must leave run_fm_pll, not only the lambda
    bool spare_moved = false;     // the passes after the second went to the side stream
    // the wrap counts and masks the lock logic's walk reads: two copies in the pipelined chain, where the walk of this call
    // runs beside the next call's front end and is not ordered before that call's PLL passes, which write them again
    const bool walk_late = p.walk_late, spare_aside = p.spare_aside;
    const int pll_iters = p.pll_iters, wpar = walk_late ? walk_par : 0;
    if (walk_late) walk_par ^= 1;
    int *const ck_wraps_now = d_ck_wraps.p + (size_t)wpar * ck_copy;
    unsigned long long *const ck_mask_now = d_ck_mask.p + (size_t)wpar * ck_copy * mask_words;
    // (trace mode: every kernel of the group carries its own event pair)
    auto sub = [&](hipStream_t st, const char *name, auto &&launch) { if (timing == 3) timed_on(st, name, launch); else launch(); };
    timed("pll", [&] {
      const int ngrp = (nck + FMR_NODE_GRP - 1) / FMR_NODE_GRP;
      const int ngrp2 = (ngrp + FMR_NODE_GRP2 - 1) / FMR_NODE_GRP2;
      hipStream_t ps = stream;
      for (int it = 0; it < pll_iters; it++) {
        if (spare_aside && it == 2 && !spare_moved) { (void)hipEventRecord(ev_pll1, stream); (void)hipStreamWaitEvent(side, ev_pll1, 0); spare_moved = true; ps = side; }
        // round 0 integrates the sensitivities too; later rounds reuse them (chord Newton: measured
        // contraction 5e-4 per round in lock, so the round count is the same as with fresh Jacobians)
        PllSync *const sy = env.pll_v1 ? nullptr : d_pll_sync.p;      // null: seven-kernel round (k_pll_check etc.)
        // The pass that integrates the Jacobians composes them in its own tail (the node pass's up-sweep: k_pll_up's work
        // without its launch and without reading 31 MB of Jacobians back), see k_pll_shoot
        const bool up_in_shoot = sy != nullptr && it < pll_jac_rounds && it + 1 < pll_iters;
        const PllUpArgs upa = up_in_shoot ? PllUpArgs{d_pll_PQ.p, d_pll_pre.p, d_pll_PQ2.p, ngrp, ngrp2, d_pll_dstart2.p, d_pll_sync.p, d_pll_tick2.p, d_pll_te.p}
                                          : PllUpArgs{};
        // ... and every later pass runs the down-sweep of the node pass before it in its own head (k_pll_down's work without
        // its launch): a round is two launches, integration + up-sweep kernel (the first round: one)
        const bool down_in_shoot = sy != nullptr && it > 0;
        // Right behind the Jacobian round the sweep is a descent through that round's tree; a chord round's mismatches are
        // new, the tree's composites are not: it keeps the chain, behind k_pll_up
        const bool descend = down_in_shoot && it == pll_jac_rounds && !env.x_pll_chain_head;
        const PllDownArgs dna = down_in_shoot ? PllDownArgs{d_pll_pre.p, d_pll_dstart2.p, ngrp, ngrp2, pllc.minfreq, pllc.maxfreq, d_pll_wfirst.p,
                                                            descend ? d_pll_te.p : (const double *)nullptr}
                                              : PllDownArgs{};
        auto shoot = [&](auto kern) {
          sub(ps, it == 0 ? "pll_shoot_jac" : "pll_shoot", [&] {
          hipLaunchKernelGGL(kern, dim3((nck + 63) / 64, S), dim3(64), 0, ps, k.base, base_stride, H_b, ct,
                             k.raw, base_stride, H_b, d_atan.p, pllc, (int)pilot_shift, d_pll_nodes.p, d_pll_G.p,
                             d_pll_M.p, ck_wraps_now, ck_mask_now, mask_words, d_flags.p, d_pll_wgr.p, sy, 1.0,
                             pll_rtol, (int)(it > 0), upa, dna, sy ? d_pll_wfirst.p : (double *)nullptr);
          });
        };
        // the first round writes no L-R samples unless it can be the accepted one (a call of one or two chunks)
        const bool wout = it > 0 || env.pll_v1 || nck <= 2;
        if (it < pll_jac_rounds) { if (wout) shoot(k_pll_shoot<true, true>); else shoot(k_pll_shoot<true, false>); }
        else shoot(k_pll_shoot<false, true>);
        if (it == 0) launch_fe_post(k.fe_post);
        if (it == 0 && k.agc_deferred) {
          // side2: the AGC and the mono audio tail beside the PLL.  Gated on an event that exists already -- the
          // front end's (ev_disc) -- because a marker of its own on this stream costs ~10 us between the first pass
          // and the node pass.
          k.agc_deferred = false;
          hipEvent_t gate = k.ev_mpx;
          if (!gate) { (void)hipEventRecord(ev_if, stream); gate = ev_if; }
          if ((rc_agc = enqueue_agc(k.agc, gate))) return;
          if (split_mono) {
            (void)hipStreamWaitEvent(side2, gate, 0);
            tail_channels(t, side2, 0, 1);
            (void)hipEventRecord(ev_mono, side2);
            t.mono_enqueued = true;
          }
        }
#ifdef FMR_AB_PARTNERS
        if (env.pll_v1)
          hipLaunchKernelGGL(k_pll_check, dim3(S), dim3(1024), 0, stream, d_flags.p, S, 1.0, d_pll_gres.p, ngrp,
                             (int)(it > 0), d_pll_wgr.p, (nck + 63) / 64, pll_rtol);
#endif
        if (it == pll_iters - 1) break;        // nothing integrates the nodes a last update would give
        if (!env.pll_v1) {
          if (!up_in_shoot) {
          if (spare_aside && it == 1) { (void)hipEventRecord(ev_pll1, stream); (void)hipStreamWaitEvent(side, ev_pll1, 0); spare_moved = true; ps = side; }
          sub(ps, "pll_up", [&] {
          hipLaunchKernelGGL(k_pll_up, dim3(ngrp, S), dim3(64), 0, ps, d_pll_nodes.p, d_pll_G.p, d_pll_M.p, nck,
                             d_pll_PQ.p, d_pll_pre.p, d_pll_PQ2.p, ngrp2, d_pll_dstart2.p, d_flags.p, d_pll_sync.p,
                             d_pll_tick2.p);
          });
          }
          continue;
        }
#ifdef FMR_AB_PARTNERS
        hipLaunchKernelGGL(k_pll_nodes_a, dim3(ngrp, S), dim3(64), 0, stream, d_pll_nodes.p, d_pll_G.p, d_pll_M.p,
                           nck, d_pll_PQ.p, d_flags.p);
        hipLaunchKernelGGL(k_pll_nodes_a2, dim3(ngrp2, S), dim3(64), 0, stream, d_pll_PQ.p, ngrp, d_pll_PQ2.p,
                           d_flags.p);
        hipLaunchKernelGGL(k_pll_nodes_b, dim3(S), dim3(64), 0, stream, d_pll_PQ2.p, ngrp2, d_pll_dstart2.p,
                           d_flags.p);
        hipLaunchKernelGGL(k_pll_nodes_c2, dim3(ngrp2, S), dim3(64), 0, stream, d_pll_PQ.p, ngrp, d_pll_dstart2.p,
                           d_pll_dstart.p, d_flags.p);
        hipLaunchKernelGGL(k_pll_nodes_c, dim3(ngrp, S), dim3(64), 0, stream, d_pll_nodes.p, d_pll_G.p, d_pll_M.p,
                           nck, d_pll_dstart.p, d_flags.p, pllc.minfreq, pllc.maxfreq, d_pll_gres.p);
#endif
      }
      // the serial fallback (a kernel that reads a flag and leaves unless the rounds gave up) goes with the lock logic in the
      // pipelined chain: it carries the lock counters on, as the late walk of the call before does on that stream
      if (walk_late && !spare_moved) { (void)hipEventRecord(ev_pll1, stream); (void)hipStreamWaitEvent(side, ev_pll1, 0); spare_moved = true; ps = side; }
      if (pilot_shift)
        hipLaunchKernelGGL(k_pll_fallback<true>, dim3(S), dim3(64), 0, ps, k.base, base_stride, H_b, bt,
                           k.raw, base_stride, H_b, d_atan.p, pllc, k.stereo_blk, d_state.p, S, d_flags.p);
      else
        hipLaunchKernelGGL(k_pll_fallback<false>, dim3(S), dim3(64), 0, ps, k.base, base_stride, H_b, bt,
                           k.raw, base_stride, H_b, d_atan.p, pllc, k.stereo_blk, d_state.p, S, d_flags.p);
    });
    if (rc_agc) return rc_agc;
    HIPCHK(hipGetLastError());    // a launch of the rounds above that could not be enqueued
    // lock logic / PPS / state commit beside the audio chain (needed again only by fm_out)
    if (spare_moved) HIPCHK(hipEventRecord(ev_pll, side));
    else {
      HIPCHK(hipEventRecord(ev_pll, stream));
      HIPCHK(hipStreamWaitEvent(side, ev_pll, 0));
    }
    // the lock logic's walk over the blocks: with the values of THIS call, whichever call enqueues it
    const WalkJob w{k.base, base_stride, bt, ct, ck_wraps_now, ck_mask_now, k.stereo_blk, d_walk_go.p + (size_t)wpar * S,
                    side_ballast(), walk_late};
    timed_on(side, walk_late ? "pll_commit" : "pll_blocks", [&] {
      hipLaunchKernelGGL(k_pll_blocks, dim3((nb + 3) / 4, S), dim3(256), w.ballast, side, bt, ct, d_pll_G.p,
                         ck_wraps_now, d_blk_wraps.p, d_blk_level.p, d_flags.p);
      if (walk_late)
        hipLaunchKernelGGL(k_pll_commit, dim3(S), dim3(FMR_COMMIT_THREADS), (env.x_ballast & 2) ? (size_t)kBallastBytes : w.ballast, side, bt, ct, pllc, d_pll_G.p, d_blk_wraps.p,
                           d_blk_level.p, d_state.p, d_flags.p, w.walk_go);
    });
    if (walk_late) {
      // (the tail waits for this stream's statistics and AGC itself: ev_fin, recorded behind the late walk, covers neither)
      walk_job = w; walk_pending = true;
      t.fin_on_side = true;
      return FMR_OK;
    }
    if (int rcw = pll_walk(w)) return rcw;
    // one event for everything beside the main stream: this stream's own work (statistics, lock logic) and the
    // AGC stream's -- the main stream then waits once, before the output mux, instead of four times
    if (k.agc_on_side && !k.agc_deferred) { HIPCHK(hipStreamWaitEvent(side, ev_agc, 0)); t.fin_covers_all = true; }
    HIPCHK(hipEventRecord(ev_fin, side));
    t.fin_on_side = true;
  }
  return FMR_OK;
}

// k_pll_finish on the side stream: lock counters, PPS events and the per-block stereo flags of the call that made the job
int fmr_chain::pll_walk(const WalkJob &w) {
  timed_on(side, "pll_finish", [&] {
    hipLaunchKernelGGL(k_pll_finish, dim3(S), dim3(64), (env.x_ballast & 1) ? (size_t)kBallastBytes : w.ballast, side, w.base, w.base_stride, H_b, w.bt, w.ct, d_atan.p,
                       pllc, (int)pilot_shift, d_pll_nodes.p, d_pll_G.p, w.ck_wraps, w.ck_mask, mask_words,
                       d_blk_wraps.p, d_blk_level.p, w.stereo_blk, d_state.p, d_flags.p,
                       w.late ? w.walk_go : (const int *)nullptr);
  });
  if (w.late) HIPCHK(hipEventRecord(ev_fin, side));
  return FMR_OK;
}

// FmDecoder: equaliser, discriminator, statistics, pilot PLL, audio resampler + tail, DC block + mux
int fmr_chain::run_fm(CallCtx &k) {
  const CallPlan &p = k.plan;
  const int nb = k.nb;
  const long long N_if = k.N_if, N_au = k.N_au; const BlockTab &bt = k.bt;
  if (k.any_mpf)
    timed("mpf", [&] {
      // the chain-and-helpers form (k_mpf4: no barrier inside a chunk)
      constexpr int NG4 = FMR_MPF_CH / 4 + 2;
      const int tpl4 = mpf_N <= 320 ? 5 : mpf_N <= 640 ? 10 : 20;      // (plan_create(): mpf_N <= kMaxMpfTaps = 1280)
      const size_t lds4 = sizeof(float2) * ((size_t)mpf_N + FMR_MPF_CH + 8) + sizeof(float) * NG4 + sizeof(float2) * FMR_MPF_CH +
                          sizeof(double) * NG4 + sizeof(float2) * (tpl4 <= 10 ? 16 : 8) * 64 * (size_t)tpl4 + sizeof(int) * 16 +
                          sizeof(float2);
      auto go4 = [&](auto kern) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds4);
        hipLaunchKernelGGL(kern, dim3(S), dim3(256), lds4, stream, k.xin, k.x_stride, k.x_off, d_gain.p, (long long)max_if,
                           bt, d_mpf.p, (long long)max_if, d_mpf_coeff.p, d_mpf_state.p, mpf_N, mpf_ref,
                           d_mpf_ok.p, d_state.p, agc_beside_mpf ? d_agc_progress.p : (const unsigned long long *)nullptr,
                           kAgcWaitTicks);
      };
      if (mpf_N <= 64 * 5) go4(k_mpf4<5>);
      else if (mpf_N <= 64 * 10) go4(k_mpf4<10>);
      else go4(k_mpf4<20>);
    });
  // the discriminator multiplies the gains into the blocks the equaliser passed over (warm-up, resets), and the AGC's
  // state must be committed before the next call: the AGC kernel finished long ago (it is three times faster)
  if (agc_beside_mpf) HIPCHK(hipStreamWaitEvent(stream, ev_agc, 0));
  const long long base_stride = H_b + (long long)max_if;   // pre-de-emphasis buffers
  const long long de_stride = H_a + (long long)max_if;     // de-emphasised copies feeding the audio resampler
  if (!p.b_disc && !p.fir_disc() && !mpx_in)     // (the fused front end's / the IF filter's discriminator epilogue, or the MPX input, has already written the MPX and the block statistics)
  timed("disc", [&] {
    hipLaunchKernelGGL((k_disc<256, fm_mpx_t>), dim3(nb, S), dim3(256), 0, stream, k.xin, k.x_stride, k.x_off, k.disc_gain,
                       (long long)max_if, k.any_mpf ? d_mpf.p : (float2 *)nullptr, (long long)max_if, d_mpf_ok.p, bt,
                       disc_nf, disc_bound, d_dec.p, (long long)max_if, k.base, base_stride, H_b,
                       d_bb_mean_blk.p, d_bb_rms_blk.p, d_state.p, p.fir == IfForm::none ? d_if_rms_blk.p : (float *)nullptr);
  });
  // "the MPX is there": what the side streams start from.  Behind the fused front end on the decoder's own stream that is
  // the event recorded behind it already (a second marker on the critical stream costs what a small kernel costs).
  k.ev_mpx = (pipelined && p.b_disc) ? ev_fe[k.par] : ev_disc;
  if (k.ev_mpx == ev_disc) HIPCHK(hipEventRecord(ev_disc, stream));
  if (k.tail_deferred) { k.tail_deferred = false; if (int rc = flush_tail(ev_disc)) return rc; }
  HIPCHK(hipStreamWaitEvent(side, k.ev_mpx, 0));
  if (p.b == StageB::fused && !pipelined)      // input history for the next call's front end: off the critical path (the next
    timed_on(side, "in_halo", [&] {   // front end waits for this stream's table kernels anyway)
      hipLaunchKernelGGL((k_update_in_halo<256, 0>), dim3(1, S), dim3(256), 0, side, d_in_halo.p, H_in, k.d_iq, (long long)k.stride, k.N_in);
    });
  const size_t stats_ballast = side_ballast();
  timed_on(side, "stats", [&] {     // (fused front end: the block values are summed from its partial sums on the fly)
    hipLaunchKernelGGL(k_stats, dim3(S), dim3(FMR_STATS_THREADS), stats_ballast, side, bt, d_if_rms_blk.p, d_bb_mean_blk.p,
                       d_bb_rms_blk.p, d_state.p, S, (int)!(pipelined && p.b_disc),   // (the front-end stage commits its own phase)
                       (p.b_disc || p.fir_tail()) ? k.part : (const FusedPart *)nullptr, p.fir_tail() ? 8 * p.fir_runs.tiles : k.fused_n_tiles,
                       p.fir_tail() ? 0 : k.fused_kb_ref, out.ifrms_slot(k.par));
  });
  HIPCHK(hipEventRecord(ev_stats, side));
  disc_commit_on_side = !(pipelined && p.b_disc);
  // ---------------------------------------------------- audio resampler + tail
  TailCtx t{};
  t.ifbuf = k.ifbuf; t.if_nrm = k.nrm != nullptr;
  t.base = k.base; t.raw = k.raw; t.stereo_blk = k.stereo_blk; t.N_if = N_if; t.N_au = N_au; t.nb = nb; t.bt = bt;
  t.d_aud = k.d_aud; t.astride = (long long)k.astride; t.amA_prev = k.amA_prev; t.akB_prev = k.akB_prev;
  t.nch = stereo ? 2 : 1;
  if (out.on) { t.out = out.begin(k.out_block0, k.tab.if_len, nb, N_au); t.out_ifrms = out.ifrms_slot(k.par); }
  if (ws.on) t.ws = ws.begin(N_if, N_au);
  if (mpxo.on) t.mpxo = mpxo.begin(N_if);
  for (int b = 0; b < nb; b++) t.au_max = std::max(t.au_max, k.tab.au_len[b]);
  t.count_am = (int)(arsc.mA - k.amA_prev);
  if ((size_t)t.count_am > max_amid || (size_t)N_au > max_au) { set_err("internal audio capacity exceeded"); return FMR_ERR_CAPACITY; }
  t.a_top0 = (long long)ars.D * k.amA_prev + ars.ca() - k.an_prev;
  // fused de-emphasis + stage A: the tile (warm-up + (TOUT-1) D + NA samples) must fit BLOCK * LPL LDS slots;
  // at most 4 * DE_BLOCK outputs per tile: every lane then owns exactly one run of 4 outputs in the FIR phase
  t.de_tout = std::min(4 * kDeBlock, ((kDeBlock * FMR_DE_LPL - FMR_DE_WARMUP - ars.NA - ars.D) / ars.D) & ~3);
  t.de_fused = !env.serial && t.de_tout >= 64;
  t.dc_nc = (int)((N_au + C_DC - 1) / C_DC);
  t.dk = dk;
  const long long am_stride = H_am + (long long)max_amid;
  const long long a1_stride = H_pc + (long long)max_au;
  // Channel 0 (mono = L+R) does not depend on the PLL: in the in-order chain with stereo on it runs on the AGC stream while
  // the PLL iterates, and only L-R stays behind the PLL on the decoder stream.  In the pipelined chain both channels belong
  // to the tail STAGE (its own stream, a call behind the PLL stage): the mono channel's buffers are still being read by the
  // previous call's DC block and mux while this call's PLL iterates.
  t.can_split = stereo && !env.serial && t.de_fused && (ars.LB == 3 && ars.MB == 8) && n_pilotcut <= FMR_PCUT_MAXTAPS;
  t.ev_mpx = k.ev_mpx;
  if (stereo) if (int rcp = run_fm_pll(k, t)) return rcp;
  if (k.agc_deferred) { k.agc_deferred = false; if (int rca = enqueue_agc(k.agc, nullptr)) return rca; }   // PLL path not taken
  launch_fe_post(k.fe_post);
  t.agc_on_side = k.agc_on_side;
  if (!pipelined) {
    if (fir_enable) k.add_halo(k.ifbuf, k.if_stride, H_if, N_if);
    k.add_halo(k.base, base_stride, H_b, N_if, 1);
    if (stereo) k.add_halo(k.raw, base_stride, H_b, N_if);
  }       // (pipelined: the halos of the ring slots are carried over at the head of the next call, run_tables)
  if (!t.de_fused || env.debug_taps) {     // (the fused de-emphasis keeps the 384 kHz signal in LDS: these are taps then)
    k.add_halo(d_base_de.p, de_stride, H_a, N_if);
    if (stereo) k.add_halo(d_raw_de.p, de_stride, H_a, N_if);
  }
  k.add_halo(d_am0.p, am_stride, H_am, t.count_am);
  if (stereo) k.add_halo(d_am1.p, am_stride, H_am, t.count_am);
  k.add_halo(d_a10.p, a1_stride, H_pc, N_au);
  if (stereo) k.add_halo(d_a11.p, a1_stride, H_pc, N_au);
  if (k.audio_len) for (int b = 0; b < nb; b++) k.audio_len[b] = (uint32_t)(stereo ? 2 * k.tab.au_len[b] : k.tab.au_len[b]);
  if (pipelined) {
    // end of the PLL stage on the decoder stream: the tail of this call starts from it.  The tail stage itself is enqueued behind the NEXT call's front end (or by whatever
    // synchronises the chain first): it then runs beside that call's PLL stage and leaves the front end the whole chip.
    if (!stereo) HIPCHK(hipEventRecord(ev_pll, stream));
    t.ht = k.ht; k.ht.n = 0; t.seq = pipe_seq;
    tail_job = t; tail_pending = true;
    return FMR_OK;
  }
  return tail_stage(t, stream);
}

// Per-channel part of the audio tail (de-emphasis + audio resampler + pilot cut + DC-block pass 1) for channels
// ch_base .. ch_base + nch_l - 1 on stream st.
void fmr_chain::tail_channels(const TailCtx &t, hipStream_t st, int ch_base, int nch_l) {
  const long long base_stride = H_b + (long long)max_if, de_stride = H_a + (long long)max_if;
  const long long am_stride = H_am + (long long)max_amid, a1_stride = H_pc + (long long)max_au;
  const int count_am = t.count_am, de_tout = t.de_tout, dc_nc = t.dc_nc;
  const long long N_if = t.N_if, N_au = t.N_au, a_top0 = t.a_top0, amA_prev = t.amA_prev, akB_prev = t.akB_prev;
  const BlockTab &bt = t.bt;
  const int nb = t.nb;
  constexpr int DE_BLOCK = kDeBlock, DE_SLOTS = DE_BLOCK * FMR_DE_LPL;
  if (t.de_fused) {
    if (count_am > 0) {
      timed_on(st, "deemph_decim", [&] {
        const int tiles = (count_am + de_tout - 1) / de_tout;
        const size_t lds = sizeof(double) * (size_t)(DE_BLOCK * FMR_DE_RUN + 1);      // (an even run length carries a pad word: de_idx)
        auto go = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3(tiles, S, nch_l), dim3(DE_BLOCK), lds, st, t.base, t.raw, base_stride, H_b,
                             (int)N_if, deemph.b0, deemph.a1, de_scan, 1, (int)(stereo && !pilot_shift), d_ahA.p,
                             ars.NA, ars.D, a_top0, count_am, de_tout, d_am0.p, d_am1.p, am_stride, H_am,
                             env.debug_taps ? d_base_de.p : (double *)nullptr,
                             env.debug_taps ? d_raw_de.p : (double *)nullptr, de_stride, H_a, ch_base);
        };
        if (ars.NA == 59 && ars.D == 3) go(k_deemph_decim<DE_BLOCK, 59, 3>);     // 384 kHz -> 48 kHz
        else go(k_deemph_decim<DE_BLOCK, 0, 0>);
      });
    }
  } else {
    // ---- de-emphasis by warm-up, out of place: base/raw -> base_de/raw_de
    timed_on(st, "deemph", [&] {
      const int nt = (int)((N_if + C_DE - 1) / C_DE);
      hipLaunchKernelGGL(k_deemph_par<C_DE>, dim3((nt + 63) / 64, S, nch_l), dim3(64), 0, st, t.base, t.raw,
                         base_stride, H_b, d_base_de.p, d_raw_de.p, de_stride, H_a, (int)N_if, deemph.b0, deemph.a1, 1,
                         (int)(stereo && !pilot_shift));
    });
    if (count_am > 0) {
      timed_on(st, "aud_decim", [&] {
        hipLaunchKernelGGL(k_aud_decim<128>, dim3((count_am + 127) / 128, S, nch_l), dim3(128), 0, st, d_base_de.p,
                           d_raw_de.p, de_stride, H_a, d_ahA.p, ars.NA, ars.D, a_top0, count_am, d_am0.p, d_am1.p,
                           am_stride, H_am);
      });
    }
  }
  if (N_au > 0) {
    timed_on(st, "aud_poly", [&] {
      if (ars.LB == 3 && ars.MB == 8) {
        // period form: one lane per period (3 outputs), taps through the scalar cache
        constexpr int BLP = 256;
        const long long P_first = akB_prev / 3, P_last = (akB_prev + N_au - 1) / 3;
        const int tiles = (int)((P_last - P_first) / BLP + 1);
        const int lx = (BLP - 1) * (int)ars.MB + (int)((2 * ars.MB) / 3) + ars.TB;
        int ni_pad = (lx + (int)ars.MB - 1) / (int)ars.MB + 1;
        if ((ni_pad & 1) == 0) ni_pad++;
        hipLaunchKernelGGL((k_aud_poly2<BLP, 3, 8>), dim3(tiles, S, nch_l), dim3(BLP), sizeof(double) * (size_t)ars.MB * ni_pad,
                           st, d_am0.p, d_am1.p, am_stride, amA_prev - H_am, d_ahB.p, ars.TB,
                           akB_prev, (int)N_au, d_a10.p, d_a11.p, a1_stride, H_pc, ni_pad, H_am + count_am, ch_base);
      } else {
        hipLaunchKernelGGL(k_aud_poly<128>, dim3((unsigned)((N_au + 127) / 128), S, nch_l), dim3(128), 0, st,
                           d_am0.p, d_am1.p, am_stride, amA_prev - H_am, d_ahB.p, ars.TB, (unsigned)ars.LB,
                           (unsigned)ars.MB, (unsigned long long)akB_prev * ars.MB, (int)N_au, d_a10.p, d_a11.p,
                           a1_stride, H_pc);
      }
    });
    timed_on(st, "pilotcut", [&] {
      // (a 65536-sample block is 314 or 315 audio samples: the one-tile form takes 4.6 KB of LDS instead of 12.3, and thirteen
      // instead of five of its workgroups fit beside a PLL pass on a compute unit)
      if (n_pilotcut <= FMR_PCUT_MAXTAPS && t.au_max <= 320)
        hipLaunchKernelGGL((k_pilotcut2<320, 320>), dim3(nb, S, nch_l), dim3(320), 0, st, d_a10.p, d_a11.p,
                           a1_stride, H_pc, bt, d_pilotcut.p, n_pilotcut, d_pc0.p, d_pc1.p, (long long)max_au, 1.0, ch_base);
      else if (n_pilotcut <= FMR_PCUT_MAXTAPS)
        hipLaunchKernelGGL((k_pilotcut2<320, 1280>), dim3(nb, S, nch_l), dim3(320), 0, st, d_a10.p, d_a11.p,
                           a1_stride, H_pc, bt, d_pilotcut.p, n_pilotcut, d_pc0.p, d_pc1.p, (long long)max_au, 1.0, ch_base);
      else
        hipLaunchKernelGGL(k_pilotcut<128>, dim3(nb, S, nch_l), dim3(128), 0, st, d_a10.p, d_a11.p, a1_stride, H_pc,
                           bt, d_pilotcut.p, n_pilotcut, d_pc0.p, d_pc1.p, (long long)max_au);
    });
  }
  if (N_au > 0 && !env.serial)
    timed_on(st, "dc_pass1", [&] {
      hipLaunchKernelGGL(k_dc_pass1<C_DC>, dim3((dc_nc + 63) / 64, S, nch_l), dim3(64), 0, st, d_pc0.p, d_pc1.p,
                         (long long)max_au, (int)N_au, t.dk, d_dc_G.p, dc_nc, ch_base);
    });
}

// The audio tail of one call on stream ts: the channels the PLL stage has not already run beside itself, the DC block's
// node pass, the output mux, and the joins with what ran beside the decoder stream (statistics, AGC, lock logic).
int fmr_chain::tail_stage(const TailCtx &t, hipStream_t ts) {
  if (rds.on) if (int rc = rds_stage(t.base, t.N_if, ts)) return rc;
  if (mon.on)
    if (int rc = seg_stage(mon, t.base, H_b + (long long)max_if, H_b, (float)mon.hist_range,
                           (float)((double)mon.bins / (2.0 * mon.hist_range)), k_mon_seg<MonMpxSrc>,
                           k_mon_reduce<MonMpxSrc>, "mon_seg", "mon_reduce", t.N_if, ts))
      return rc;
  if (rfm.on)      // (the IF ring slot holds IF samples, or |x|^2 when if_nrm; the integer bin rule takes no range)
    if (int rc = seg_stage(rfm, t.ifbuf, H_if + (long long)max_if, H_if, 0.f, 0.f,
                           t.if_nrm ? k_mon_seg<RfmSrc<true>> : k_mon_seg<RfmSrc<false>>,
                           t.if_nrm ? k_mon_reduce<RfmSrc<true>> : k_mon_reduce<RfmSrc<false>>, "rfm_seg", "rfm_reduce",
                           t.N_if, ts))
      return rc;
  if (ws.on) if (int rc = ws_measure(t.base, t.ws, ts)) return rc;
  if (mpxo.on) if (int rc = mpxout_stage(t.base, t.mpxo, ts)) return rc;
  const int nch = t.nch, dc_nc = t.dc_nc;
  const long long N_au = t.N_au;
  if (t.mono_enqueued) tail_channels(t, ts, 1, 1);
  else tail_channels(t, ts, 0, nch);
  if (t.mono_enqueued) HIPCHK(hipStreamWaitEvent(ts, ev_mono, 0));   // DC-block node pass needs both channels
  if (N_au > 0) {
    if (t.fin_on_side && env.serial) HIPCHK(hipStreamWaitEvent(ts, ev_fin, 0));
    if (env.serial) {
      timed_on(ts, "fm_out", [&] {
        hipLaunchKernelGGL(k_fm_out, dim3(S), dim3(64), 0, ts, d_pc0.p, d_pc1.p, (long long)max_au, t.bt, (int)N_au,
                           dcblock.b0, dcblock.b1, dcblock.b2, dcblock.a1, dcblock.a2, (int)stereo, (int)pilot_shift,
                           t.stereo_blk, t.d_aud, t.astride, d_state.p);
      });
    } else {
      // ---- DC block by linear multiple shooting + output mux
      timed_on(ts, "fm_out", [&] {
        const int dc_nw = std::max(1, std::min(FMR_DC_MAXW, (dc_nc + 64 * FMR_DC_K - 1) / (64 * FMR_DC_K)));
        hipLaunchKernelGGL(k_dc_nodes, dim3(S * nch), dim3(64 * dc_nw), 0, ts, d_dc_G.p, d_dc_start.p, dc_nc, t.dk,
                           d_state.p, S, nch);
        if (t.fin_on_side) (void)hipStreamWaitEvent(ts, ev_fin, 0);   // only the mux needs the lock flags
        hipLaunchKernelGGL(k_dc_pass2_mux<C_DC>, dim3((dc_nc + 63) / 64, S), dim3(64), 0, ts, d_pc0.p, d_pc1.p,
                           (long long)max_au, t.bt, (int)N_au, t.dk, d_dc_start.p, dc_nc, (int)stereo, (int)pilot_shift,
                           t.stereo_blk, t.d_aud, t.astride, d_state.p);
      });
    }
  }
  if (ws.on && ws.cfg.mode == FMR_WS_ACT) if (int rc = ws_act(t.d_aud, t.astride, t.ws, ts)) return rc;
  if (ld.on) if (int rc = ld_stage(t.d_aud, t.astride, N_au, ts)) return rc;
  if (an.on) if (int rc = an_stage(t.d_aud, t.astride, N_au, ts)) return rc;
  if (!(t.fin_covers_all && N_au > 0)) {        // (otherwise the wait before the output mux covered all three)
    HIPCHK(hipStreamWaitEvent(ts, ev_stats, 0));
    if (t.agc_on_side) HIPCHK(hipStreamWaitEvent(ts, ev_agc, 0));
    if (t.fin_on_side) HIPCHK(hipStreamWaitEvent(ts, ev_fin, 0));
  }
  if (out.on) if (int rc = out_stage(t.d_aud, t.astride, t.bt, t.out_ifrms, t.out, ts)) return rc;   // (behind the statistics: ev_stats)
  return FMR_OK;
}

// ---- RDS stage (kernels_rds.hpp) ----
// Taps: h1 = Blackman-windowed sinc, cut-off 12 kHz at 384 kHz (flat to 3.7 kHz, -74 dB from 20.3 kHz on, where the
// 24 kHz output would alias into the RDS band); h2 = the standard's shaping filter cos(pi f td / 4), |f| < 2 / td, whose
// impulse response is p(t) = cos(4 pi t / td) / (1 - (8 t / td)^2), sampled at 24 kHz over +-2 symbols.
static double rds_pulse(double t) {
  const double td = 1.0 / 1187.5, u = 8.0 * t / td;
  if (std::fabs(std::fabs(u) - 1.0) < 1e-9) return M_PI / 4.0;
  return std::cos(M_PI * u / 2.0) / (1.0 - u * u);
}
int RdsStage::init(int streams, size_t max_if) {
  S = streams;
  const size_t need = max_if / kRdsD + 5 * 1300 + 256;
  R = 1;
  while ((size_t)R < need) R <<= 1;
  maxw = (int)(((double)max_if * 19.0) / (double)(kRdsWin * kRdsSym)) + 3;
  std::vector<float> h1(kRdsNT1), h2(kRdsNT2);
  double sum = 0.0;
  std::vector<double> hd(kRdsNT1);
  for (int k = 0; k < kRdsNT1; k++) {
    const double x = k - (kRdsNT1 - 1) / 2.0, fc = 12000.0 / kFmRate;
    const double sinc = 2.0 * fc * (x == 0.0 ? 1.0 : std::sin(2.0 * M_PI * fc * x) / (2.0 * M_PI * fc * x));
    const double w = 0.42 - 0.5 * std::cos(2.0 * M_PI * k / (kRdsNT1 - 1)) + 0.08 * std::cos(4.0 * M_PI * k / (kRdsNT1 - 1));
    hd[k] = sinc * w;
    sum += hd[k];
  }
  for (int k = 0; k < kRdsNT1; k++) h1[k] = (float)(hd[k] / sum);
  const double fs2 = kFmRate / kRdsD, T = 0.5 / 1187.5;
  for (int j = 0; j < kRdsNT2; j++) h2[j] = (float)rds_pulse((j - (kRdsNT2 - 1) / 2) / fs2);
  // soft symbol of one isolated symbol of a unit subcarrier: the mixer halves it, z = d / 2 with d(t) = p(t) - p(t - T)
  auto d = [&](double t) { return rds_pulse(t) - rds_pulse(t - T); };
  double y0 = 0.0, yT = 0.0;
  for (int j = 0; j < kRdsNT2; j++) {
    const double u = (j - (kRdsNT2 - 1) / 2) / fs2;
    y0 += h2[j] * 0.5 * d(-u);
    yT += h2[j] * 0.5 * d(T - u);
  }
  gain = std::fabs(y0 - yT);
  std::vector<float2> lo(128);
  for (int i = 0; i < 128; i++) lo[i] = make_float2((float)std::cos(2.0 * M_PI * i / 128.0), (float)-std::sin(2.0 * M_PI * i / 128.0));
  int rc;
  if ((rc = upload(d_h1, h1.data(), h1.size()))) return rc;
  if ((rc = upload(d_h2, h2.data(), h2.size()))) return rc;
  if ((rc = upload(d_lo, lo.data(), lo.size()))) return rc;
  if ((rc = d_xhalo.alloc((size_t)S * kRdsHalo))) return rc;
  if ((rc = d_y1.alloc((size_t)S * R))) return rc;
  if ((rc = d_y2.alloc((size_t)S * R))) return rc;
  if ((rc = d_state.alloc((size_t)S))) return rc;
  if ((rc = d_est.alloc((size_t)S * maxw))) return rc;
  if ((rc = d_rec.alloc((size_t)S * (maxw + 1)))) return rc;
  slot_stride = (rds_slot_bytes(maxw) + 63) & ~(size_t)63;
  if ((rc = h_slots.alloc(slot_stride * (size_t)S * kSlots, hipHostMallocCoherent))) return rc;
  if ((rc = h_mark.alloc(1, hipHostMallocCoherent))) return rc;
  *h_mark.p = 0;
  dec.assign(S, fmr_rds::Decoder());
  hdr.assign(S, RdsSlotHdr{});
  on = true;
  return FMR_OK;
}

// one call's MPX (N samples per stream from the base slot) through the RDS stage, on stream st
int fmr_chain::rds_stage(const fm_mpx_t *base, long long N, hipStream_t st) {
  rds.tap_seq = 0;
  if (N <= 0) return FMR_OK;
  const long long base_stride = H_b + (long long)max_if;
  const long long n0 = rds.n, m0 = (n0 + kRdsD - 1) / kRdsD, m1 = (n0 + N + kRdsD - 1) / kRdsD;
  const int cnt = (int)(m1 - m0);
  timed_on(st, "rds_mix", [&] {
    if (cnt > 0) {
      hipLaunchKernelGGL(k_rds_mix<256>, dim3((cnt + 255) / 256, S), dim3(256), 0, st, base, base_stride, H_b, rds.d_xhalo.p,
                         n0, m0, cnt, rds.d_h1.p, rds.d_lo.p, rds.d_y1.p, rds.R);
      hipLaunchKernelGGL(k_rds_mf<256>, dim3((cnt + 255) / 256, S), dim3(256), 0, st, rds.d_y1.p, rds.d_y2.p, rds.R, m0, cnt,
                         rds.d_h2.p);
    }
    hipLaunchKernelGGL(k_rds_halo, dim3(S), dim3(kRdsHalo), 0, st, base, base_stride, H_b, rds.d_xhalo.p, n0, (int)N);
  });
  rds.n = n0 + N;
  // window w is complete once the y2 sample behind its last symbol's second half (+ the interpolator's reach) is there
  auto ready = [&](long long w) {
    const double T = (double)((w + 1) * kRdsWin * kRdsSym + kRdsSym) / 19.0;
    return (long long)std::floor((T + kRdsDelay1) / kRdsD + kRdsDelay2) + 3 <= m1;
  };
  int nw = 0;
  while (nw < rds.maxw && ready(rds.w + nw)) nw++;
  if (nw == 0) { HIPCHK(hipGetLastError()); return FMR_OK; }
  const unsigned long long seq = ++rds.seq;
  if (seq > (unsigned long long)rds.kSlots) {      // the slot's previous call must have been drained
    if (int rc = wait_mark(rds.h_mark.p, seq - rds.kSlots)) return rc;
    rds.drain();
  }
  char *slot = rds.h_slots.p + (size_t)(seq % rds.kSlots) * S * rds.slot_stride;
  timed_on(st, "rds_sym", [&] {
    hipLaunchKernelGGL(k_rds_est, dim3(nw, S), dim3(64), 0, st, rds.d_y2.p, rds.R, rds.w, rds.d_est.p, rds.maxw);
    hipLaunchKernelGGL(k_rds_scan, dim3((S + 63) / 64), dim3(64), 0, st, rds.d_est.p, nw, rds.w, rds.maxw, rds.d_state.p,
                       rds.d_rec.p, slot, rds.slot_stride, S);
    hipLaunchKernelGGL(k_rds_bits, dim3(nw, S), dim3(128), 0, st, rds.d_y2.p, rds.R, rds.d_rec.p, rds.maxw, slot,
                       rds.slot_stride);
  });
  hipLaunchKernelGGL(k_signal_host, dim3(1), dim3(1), 0, st, rds.h_mark.p, seq);
  rds.w += nw;
  rds.tap_seq = seq;
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- modulation monitor and RF monitor (kernels_monitor.hpp, kernels_rfmon.hpp) ----
int SegMonitor::init(int S, size_t max_if, unsigned interval_samples, int hist_bins, double range, int max_records) {
  static_assert(sizeof(MonRec) == sizeof(fmr_monitor_record), "MonRec is fmr_monitor_record");
  static_assert(sizeof(MonRec) == sizeof(fmr_rf_monitor_record), "MonRec is fmr_rf_monitor_record");
  static_assert(offsetof(fmr_monitor_record, segments) == offsetof(MonRec, segments) &&
                offsetof(fmr_rf_monitor_record, segments) == offsetof(MonRec, segments), "the segment count of a record");
  static_assert(kRfmBins == FMR_RF_HIST_BINS && kMonPsd == FMR_RF_PSD_BINS, "the header's sizes");
  interval = interval_samples;
  bins = hist_bins;
  hist_range = range;
  ws = welch_size(kMonH, interval, max_if, kMonSubMin, kMonSubMax, 512, 1024);
  const WelchTables t = welch_tables(kMonN, kWelchHann);
  sumw2 = t.sumw2;
  const size_t B = (size_t)bins, L = (size_t)max_records, rows = (size_t)S * ws.rmax;
  int rc;
  if ((rc = upload_welch(t, d_win, d_tw))) return rc;
  if ((rc = alloc_all(d_carry, (size_t)S * kMonN, d_ppsd, rows * kMonPsd, d_phist, rows * B, d_prec, rows,
                      d_open_psd, 2 * (size_t)S * kMonPsd, d_open_hist, 2 * (size_t)S * B, d_open_rec, 2 * (size_t)S,
                      d_ring_psd, (size_t)S * L * kMonPsd, d_ring_hist, (size_t)S * L * B, d_ring_rec, (size_t)S * L)))
    return rc;
  cur.reset(S, max_records);
  on = true;
  return FMR_OK;
}

// One call's N samples per stream through a stage of the Welch segment engine (FFT size fft, hop `hop`): the segments whose
// last sample the call delivers, in launches of at most w.rmax runs per stream.  `a` carries the launch's fields to the
// kernels; seg(runs) launches the segment kernel, reduce(runs, nrec, n1, last) the reduce kernel, which refreshes the
// carry in the call's last launch (that one may have no segment: runs = 0).
template <class Args, class Seg, class Reduce>
static void welch_call(WelchSched &w, Args &a, int fft, int hop, long long N, Seg &&seg, Reduce &&reduce) {
  const long long n1 = w.n + N;
  const long long j_hi = n1 >= fft ? (n1 - fft) / hop + 1 : 0;
  a.n0 = w.n; a.spr = w.spr; a.sub = w.sub; a.sb = w.sb;
  long long j = w.next_seg;
  do {
    const WelchLaunch p = welch_plan(w.spr, w.sub, w.sb, w.rmax, j, j_hi);
    a.a0 = j; a.a1 = p.a1; a.g0 = p.g0;
    if (p.runs > 0) seg(p.runs);
    j = p.a1;
    reduce(p.runs, p.nrec, n1, (int)(j >= j_hi));
    if (p.runs > 0) w.par ^= 1;
  } while (j < j_hi);
  w.next_seg = std::max(w.next_seg, j_hi);
  w.n = n1;
}

// One call's samples (N per stream: the MPX in the base slot, or the decoder's input in the IF ring slot) through monitor
// m, on stream st.
int fmr_chain::seg_stage(SegMonitor &m, const void *from, long long stride, int off, float rf, float scale, MonSegFn kseg,
                         MonReduceFn kreduce, const char *seg_name, const char *reduce_name, long long N, hipStream_t st) {
  if (N <= 0) return FMR_OK;
  MonArgs a{};
  a.bins = m.bins; a.rf = rf; a.scale = scale;
  const int L = (int)m.cur.L, rmax = m.ws.rmax;
  const long long M = (long long)m.interval;
  welch_call(m.ws, a, kMonN, kMonH, N,
    [&](int runs) {
      timed_on(st, seg_name, [&] {
        hipLaunchKernelGGL(kseg, dim3(runs, S), dim3(kMonT), 0, st, from, stride, off, m.d_carry.p, a, m.d_win.p, m.d_tw.p,
                           rmax, m.d_ppsd.p, m.d_phist.p, m.d_prec.p);
      });
    },
    [&](int runs, int nrec, long long n1, int last) {
      timed_on(st, reduce_name, [&] {
        hipLaunchKernelGGL(kreduce, dim3(nrec, S), dim3(kMonT), 0, st, m.d_ppsd.p, m.d_phist.p, m.d_prec.p, runs, rmax, a, L,
                           M, m.ws.par, m.d_open_psd.p, m.d_open_hist.p, m.d_open_rec.p, m.d_ring_psd.p, m.d_ring_hist.p,
                           m.d_ring_rec.p, from, stride, off, m.d_carry.p, n1, last);
      });
    });
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- audio monitor (kernels_loudness.hpp) ----
int LoudnessStage::init(int S, size_t max_au, const fmr_loudness_config &m) {
  static_assert(sizeof(LdRec) == sizeof(fmr_loudness_record), "LdRec is fmr_loudness_record");
  cfg = m;
  const int Q = (int)m.step_samples;
  cps = (Q + kLdC - 1) / kLdC;
  // a call's runs: its whole chunks, one more per sub-block it touches, one at either end
  rmax = (int)std::min<size_t>(kLdMaxRuns, max_au / kLdC + max_au / Q + 4);
  // BS.1770-4 K-weighting at 48 kHz: the shelf, then the high-pass
  coef.b0[0] = 1.53512485958697; coef.b1[0] = -2.69169618940638; coef.b2[0] = 1.19839281085285;
  coef.a1[0] = -1.69065929318241; coef.a2[0] = 0.73248077421585;
  coef.b0[1] = 1.0; coef.b1[1] = -2.0; coef.b2[1] = 1.0;
  coef.a1[1] = -1.99004745483398; coef.a2[1] = 0.99007225036621;
  // A: one step of the recurrence itself on the unit states (column j = the state after e_j), then A^(2^b) by squaring
  std::vector<double> pw((size_t)kLdPow * 16);
  for (int j = 0; j < 4; j++) {
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    z[j] = 1.0;
    (void)ld_step(coef, 0.0, z);
    for (int i = 0; i < 4; i++) pw[(size_t)i * 4 + j] = z[i];
  }
  for (int b = 1; b < kLdPow; b++) {
    const double *x = &pw[(size_t)(b - 1) * 16];
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        long double acc = 0.0L;
        for (int k = 0; k < 4; k++) acc += (long double)x[i * 4 + k] * (long double)x[k * 4 + j];
        pw[(size_t)b * 16 + i * 4 + j] = (double)acc;
      }
  }
  // true peak: g_p[k] = sinc(k - p/4) (0.5 + 0.5 cos(pi (k - p/4) / 6)), p = 1 .. 3, k = -5 .. 6
  std::vector<double> taps(3 * kLdTaps);
  for (int p = 1; p < 4; p++)
    for (int k = -5; k <= 6; k++) {
      const double t = (double)k - (double)p / 4.0;
      const double u = M_PI * t;
      taps[(size_t)(p - 1) * kLdTaps + (k + 5)] = (std::sin(u) / u) * (0.5 + 0.5 * std::cos(u / 6.0));
    }
  const size_t L = (size_t)m.max_records, rows = (size_t)S * 2 * rmax;
  int rc;
  if ((rc = upload(d_pw, pw.data(), pw.size()))) return rc;
  if ((rc = upload(d_taps, taps.data(), taps.size()))) return rc;
  if ((rc = d_G.alloc(rows * 4))) return rc;
  if ((rc = d_start.alloc(rows * 4))) return rc;
  if ((rc = d_pkw.alloc(rows))) return rc;
  if ((rc = d_part.alloc((size_t)S * rmax))) return rc;
  if ((rc = d_state.alloc((size_t)S * 2 * 4))) return rc;
  if ((rc = d_hist.alloc((size_t)S * 2 * kLdHist))) return rc;
  if ((rc = d_open.alloc(2 * (size_t)S))) return rc;
  if ((rc = d_ring.alloc((size_t)S * L))) return rc;
  cur.reset(S, m.max_records);
  n = 0;
  par = 0;
  on = true;
  return FMR_OK;
}

// one call's audio (N samples per channel and stream, where the mux wrote them) through the audio monitor, on stream st,
// in launches of at most ld.rmax runs per stream
int fmr_chain::ld_stage(const double *d_aud, long long astride, long long N, hipStream_t st) {
  if (N <= 0) return FMR_OK;
  LdArgs a{};
  a.n0 = ld.n; a.Q = (int)ld.cfg.step_samples; a.cps = ld.cps; a.ch = stereo ? 2 : 1;
  const long long n1 = ld.n + N;
  auto chunk_of = [&](long long p) { const long long q = p / a.Q; return q * a.cps + (p - q * a.Q) / kLdC; };
  long long p = ld.n;
  while (p < n1) {
    a.a0 = p; a.g0 = chunk_of(p);
    long long lo, hi;
    ld_chunk(a.Q, a.cps, a.g0 + ld.rmax - 1, lo, hi);
    a.a1 = std::min(n1, hi);
    const int runs = (int)(chunk_of(a.a1 - 1) - a.g0 + 1);
    const int nrec = (int)((a.a1 - 1) / a.Q - a.a0 / a.Q + 1);
    const int lanes = runs * a.ch;
    timed_on(st, "ld_nodes", [&] {
      hipLaunchKernelGGL(k_ld_pass1, dim3((lanes + 63) / 64, S), dim3(64), 0, st, d_aud, astride, a, ld.coef, runs, ld.rmax,
                         ld.d_G.p);
      hipLaunchKernelGGL(k_ld_nodes, dim3(S * a.ch), dim3(64), 0, st, ld.d_G.p, ld.d_start.p, a, runs, ld.rmax, ld.d_pw.p,
                         ld.d_state.p);
    });
    timed_on(st, "ld_pass2", [&] {
      hipLaunchKernelGGL(k_ld_pass2, dim3((lanes + 63) / 64, S), dim3(64), 0, st, d_aud, astride, a, ld.coef, runs, ld.rmax,
                         ld.d_start.p, ld.d_pkw.p, ld.d_state.p);
    });
    timed_on(st, "ld_block", [&] {
      hipLaunchKernelGGL(k_ld_block, dim3(runs, S), dim3(kLdC), 0, st, d_aud, astride, a, ld.rmax, ld.d_taps.p, ld.d_hist.p,
                         ld.d_part.p);
    });
    timed_on(st, "ld_reduce", [&] {
      hipLaunchKernelGGL(k_ld_reduce, dim3(nrec, S), dim3(64), 0, st, ld.d_pkw.p, ld.d_part.p, runs, ld.rmax, a,
                         (int)ld.cfg.max_records, ld.par, ld.d_open.p, ld.d_ring.p, d_aud, astride, ld.d_hist.p,
                         (int)(a.a1 >= n1));
    });
    ld.par ^= 1;
    p = a.a1;
  }
  ld.n = n1;
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- weak-signal handling (kernels_weaksignal.hpp) ----
// the detector's taps (fmr_filter_table "ws_usn"): delta - (Blackman-windowed sinc, cut-off 110 kHz at 384 kHz, sum 1)
static const double *ws_taps() {
  static const std::array<double, kWsTaps> h = [] {
    std::array<double, kWsTaps> lp{};
    const double fc = 110000.0 / kFmRate;
    double sum = 0.0;
    for (int k = 0; k < kWsTaps; k++) {
      const double x = 2.0 * fc * (double)(k - 31);
      const double sinc = k == 31 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
      const double w = 0.42 - 0.5 * std::cos(2.0 * M_PI * (double)k / 62.0) + 0.08 * std::cos(4.0 * M_PI * (double)k / 62.0);
      lp[k] = 2.0 * fc * sinc * w;
      sum += lp[k];
    }
    for (int k = 0; k < kWsTaps; k++) lp[k] = (k == 31 ? 1.0 : 0.0) - lp[k] / sum;
    return lp;
  }();
  return h.data();
}

int WeakSignalStage::init(int S, size_t max_if, size_t max_au, const fmr_weak_signal_config &m) {
  static_assert(sizeof(WsRec) == sizeof(fmr_weak_signal_record), "WsRec is fmr_weak_signal_record");
  static_assert(offsetof(WsRec, usn_sum) == offsetof(fmr_weak_signal_record, usn_sum), "the doubles of a record");
  cfg = m;
  coef.c_att = 1.0 - std::exp(-2.0 / m.attack_ms);
  coef.c_rel = 1.0 - std::exp(-2.0 / m.release_ms);
  const double lo[3] = {m.blend_lo_db, m.highcut_lo_db, m.mute_lo_db}, hi[3] = {m.blend_hi_db, m.highcut_hi_db, m.mute_hi_db};
  const unsigned bit[3] = {FMR_WS_BLEND, FMR_WS_HIGHCUT, FMR_WS_MUTE};
  for (int a = 0; a < 3; a++) { coef.lo[a] = lo[a]; coef.hi[a] = hi[a]; coef.on[a] = (m.actions & bit[a]) != 0; }
  coef.R = m.record_intervals; coef.L = m.max_records;
  alpha = 1.0 - std::exp(-2.0 * M_PI * m.highcut_hz / 48000.0);
  drop = 1.0 - std::pow(10.0, m.mute_floor_db / 20.0);
  // a call touches its whole intervals and one more at either end; the ring keeps the call's intervals and the few the
  // audio still lags behind (ws_act checks both ends)
  pmax = (int)(max_if / kWsQ + 2);
  rmax = (int)(max_au / kWsA + 2);
  cring = 64;
  while ((size_t)cring < (size_t)pmax + 64) cring <<= 1;
  // beta = one step of the recurrence itself on the unit state, then beta^(2^b) by squaring
  std::vector<double> pw(kWsPow);
  pw[0] = 1.0 + alpha * (0.0 - 1.0);
  for (int b = 1; b < kWsPow; b++) pw[b] = pw[b - 1] * pw[b - 1];
  int rc;
  if ((rc = upload(d_h, ws_taps(), (size_t)kWsTaps))) return rc;
  if ((rc = upload(d_pw, pw.data(), pw.size()))) return rc;
  if ((rc = d_hist.alloc((size_t)S * kWsHist))) return rc;
  if ((rc = d_part.alloc((size_t)S * pmax))) return rc;
  if ((rc = d_state.alloc((size_t)S))) return rc;
  if ((rc = d_ctl.alloc((size_t)S * cring))) return rc;
  if ((rc = d_ring.alloc((size_t)S * (size_t)m.max_records))) return rc;
  if (m.mode == FMR_WS_ACT) {
    if ((rc = d_G.alloc((size_t)S * 2 * rmax))) return rc;
    if ((rc = d_start.alloc((size_t)S * 2 * rmax))) return rc;
  }
  cur.reset(S, m.max_records);
  n = f = 0;
  on = true;
  return FMR_OK;
}

// one call's MPX (the samples [a.n0, a.n1) of every stream, in the base slot) through the detector and the control
int fmr_chain::ws_measure(const fm_mpx_t *base, const WsArgs &a, hipStream_t st) {
  if (a.n1 <= a.n0) return FMR_OK;
  const long long tiles = (a.n1 - 1) / kWsQ - a.n0 / kWsQ + 1, base_stride = H_b + (long long)max_if;
  if (tiles > ws.pmax) { set_err("internal: a call of %lld MPX samples has more control intervals than the weak-signal stage holds", a.n1 - a.n0); return FMR_ERR_CAPACITY; }
  timed_on(st, "ws_usn", [&] {
    hipLaunchKernelGGL(k_ws_usn, dim3((unsigned)tiles, S), dim3(kWsT), 0, st, base, base_stride, H_b, ws.d_hist.p, ws.d_h.p, a.n0,
                       a.n1, ws.pmax, ws.d_part.p);
  });
  timed_on(st, "ws_control", [&] {
    hipLaunchKernelGGL(k_ws_control, dim3(S), dim3(64), 0, st, ws.d_part.p, ws.pmax, a.n0, a.n1, ws.coef, ws.d_state.p, ws.d_ctl.p,
                       ws.cring - 1, ws.d_ring.p, base, base_stride, H_b, ws.d_hist.p);
  });
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// one call's audio (the frames [a.f0, a.f1) of every stream, where the mux wrote them) through the action, in place
int fmr_chain::ws_act(double *d_aud, long long astride, const WsArgs &a, hipStream_t st) {
  if (a.f1 <= a.f0) return FMR_OK;
  // Frame f takes the intervals floor(f / A) - 1 and the one before.  The audio resampler has delivered frame f only
  // after MPX sample 8 f, so Q floor(f / A) <= 8 f < n1 and the interval is complete; and the ring still holds the oldest.
  const long long done = a.n1 / kWsQ, g_lo = a.f0 / kWsA, g_hi = (a.f1 - 1) / kWsA;
  if (g_hi > done || done - (g_lo - 2) > ws.cring) {
    set_err("internal: weak-signal control intervals %lld .. %lld of the call's audio are not among the %d kept up to %lld",
            g_lo - 2, g_hi - 1, ws.cring, done - 1);
    return FMR_ERR_CAPACITY;
  }
  const int runs = (int)(g_hi - g_lo + 1);
  if (runs > ws.rmax) { set_err("internal: a call of %lld audio frames has more chunks than the weak-signal stage holds", a.f1 - a.f0); return FMR_ERR_CAPACITY; }
  WsActArgs w{};
  w.f0 = a.f0; w.f1 = a.f1; w.ch = stereo ? 2 : 1; w.cmask = ws.cring - 1; w.alpha = ws.alpha; w.drop = ws.drop;
  timed_on(st, "ws_nodes", [&] {
    hipLaunchKernelGGL(k_ws_pass1, dim3((runs + 63) / 64, S), dim3(64), 0, st, d_aud, astride, w, ws.d_ctl.p, runs, ws.rmax, ws.d_G.p);
    hipLaunchKernelGGL(k_ws_nodes, dim3(S * w.ch), dim3(64), 0, st, ws.d_G.p, ws.d_start.p, w, runs, ws.rmax, ws.d_pw.p, ws.d_state.p);
  });
  timed_on(st, "ws_pass2", [&] {
    hipLaunchKernelGGL(k_ws_pass2, dim3((runs + 63) / 64, S), dim3(64), 0, st, d_aud, astride, w, ws.d_ctl.p, runs, ws.rmax,
                       ws.d_start.p, ws.d_state.p);
  });
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- the capture stages' common part ----
int CaptureStage::init(int rows_, size_t max_in, bool act_, int record_intervals_, int max_records) {
  rows = rows_; act = act_; record_intervals = record_intervals_;
  pmax = (int)(max_in / kNbQ + 2);       // a call touches its whole intervals and one more at either end
  pitch = (max_in + 1) & ~(size_t)1;
  int rc;
  if (act)      // (a row may start one sample in, to sit on the caller's 16-byte phase, and be one sample further apart)
    for (DevBuf<float2> &b : d_rows) if ((rc = b.alloc((size_t)rows * (pitch + 1) + 2))) return rc;
  for (Event &e : ev_rec) if ((rc = e.create(hipEventDisableTiming))) return rc;
  cur.reset(rows, max_records);
  n = 0; calls = 0;
  return FMR_OK;
}

// The call's samples, pieces and parity; from the third call on the stream waits for the records kernel of two calls ago,
// which read the parts this call writes.
int CaptureStage::begin(Call &k, const char *noun, long long N_in, hipStream_t stream) {
  k.n0 = n; k.n1 = n + N_in;
  k.pieces = (int)((k.n1 - 1) / kNbQ - k.n0 / kNbQ + 1);
  if (k.pieces > pmax) { set_err("internal: a call of %lld input samples has more intervals than %s holds", N_in, noun); return FMR_ERR_CAPACITY; }
  n = k.n1;
  k.par = (int)(++calls & 1);
  if (calls > 2) HIPCHK(hipStreamWaitEvent(stream, ev_rec[k.par], 0));
  return FMR_OK;
}

// The rows an acting stage writes in this call: the same 16-byte phase as the caller's rows, row by row, so that the front
// end picks the forms it would have.  None when the stage only measures.
void CaptureStage::out_rows(Call &k, const float2 *d_iq, size_t stride) const {
  if (!act) return;
  k.ostride = (long long)(pitch + (stride & 1));
  k.out = d_rows[k.par].p + (((uintptr_t)d_iq >> 3) & 1);
}

// Behind the records kernel on the side stream; an acting stage's rows then stand for the caller's.
int CaptureStage::finish(const Call &k, hipStream_t side, const float2 *&d_iq, size_t &stride) {
  HIPCHK(hipEventRecord(ev_rec[k.par], side));
  HIPCHK(hipGetLastError());
  if (act) {
    d_iq = k.out; stride = (size_t)k.ostride;
    last_rows = k.out; last_stride = k.ostride; last_n = k.n1 - k.n0;
  }
  return FMR_OK;
}

// ---- impulse blanker (kernels_blanker.hpp) ----
int BlankerStage::init(int rows_, size_t max_in, const fmr_blanker_config &m) {
  static_assert(sizeof(NbRec) == sizeof(fmr_blanker_record), "NbRec is fmr_blanker_record");
  static_assert(offsetof(NbRec, threshold) == offsetof(fmr_blanker_record, threshold) &&
                offsetof(NbRec, peak) == offsetof(fmr_blanker_record, peak), "the fields of a record");
  cfg = m;
  coef.G = m.gate_samples; coef.M = m.max_run_samples; coef.W = m.average_intervals; coef.R = m.record_intervals;
  coef.L = m.max_records; coef.act = m.mode == FMR_NB_ACT;
  coef.g = std::pow(10.0, m.threshold_db / 10.0);
  coef.r[0] = 0.0;
  for (int c = 1; c <= kNbMaxW; c++) coef.r[c] = 1.0 / ((double)c * 281474976710656.0);
  int rc;
  if ((rc = CaptureStage::init(rows_, max_in, coef.act, m.record_intervals, m.max_records))) return rc;
  aring = 64;
  while (aring < pmax + m.average_intervals + 2) aring <<= 1;
  if ((rc = d_part.alloc((size_t)2 * rows * pmax))) return rc;
  if ((rc = d_aring.alloc((size_t)rows * aring))) return rc;
  if ((rc = d_carry.alloc((size_t)2 * rows * (coef.G + coef.M)))) return rc;
  if ((rc = d_state.alloc((size_t)rows))) return rc;
  if ((rc = d_ring.alloc((size_t)rows * (size_t)m.max_records))) return rc;
  if ((rc = ev_apply.create(hipEventDisableTiming))) return rc;
  on = true;
  return FMR_OK;
}

// One call's input rows (the samples [nb.n, nb.n + N_in) of every row at d_iq) through the blanker, in front of everything
// that reads them; in FMR_NB_ACT d_iq and stride then name the blanked rows.
int fmr_chain::nb_stage(const float2 *&d_iq, size_t &stride, long long N_in) {
  BlankerStage &b = this->nb;
  CaptureStage::Call k;
  if (int rc = b.begin(k, "the blanker", N_in, stream)) return rc;
  NbPart *part = b.d_part.p + (size_t)k.par * b.rows * b.pmax;
  b.out_rows(k, d_iq, stride);
  timed_on(stream, "nb_level", [&] {
    hipLaunchKernelGGL(k_nb_level, dim3((unsigned)k.pieces, b.rows), dim3(kNbT), 0, stream, d_iq, (long long)stride, k.n0, k.n1, b.pmax, part);
  });
  timed_on(stream, "nb_apply", [&] {
    hipLaunchKernelGGL(k_nb_apply, dim3((unsigned)k.pieces, b.rows), dim3(kNbT), 0, stream, d_iq, (long long)stride, k.out, k.ostride, k.n0, k.n1,
                       b.pmax, k.par, part, b.d_aring.p, b.aring - 1, b.d_carry.p, b.d_state.p, b.coef);
  });
  HIPCHK(hipEventRecord(b.ev_apply, stream));
  HIPCHK(hipStreamWaitEvent(side, b.ev_apply, 0));
  timed_on(side, "nb_records", [&] {
    hipLaunchKernelGGL(k_nb_records, dim3(b.rows), dim3(64), 0, side, part, b.pmax, k.n0, k.n1, b.d_state.p, b.d_ring.p, b.coef.R, b.coef.L);
  });
  return b.finish(k, side, d_iq, stride);
}

// ---- IQ correction (kernels_iqcorr.hpp) ----
int IqCorrectionStage::init(int rows_, size_t max_in, const fmr_iq_correction_config &m) {
  static_assert(sizeof(IqcRec) == sizeof(fmr_iq_correction_record), "IqcRec is fmr_iq_correction_record");
  static_assert(offsetof(IqcRec, sum_re) == offsetof(fmr_iq_correction_record, sum_re) &&
                offsetof(IqcRec, n_intervals) == offsetof(fmr_iq_correction_record, n_intervals) &&
                offsetof(IqcRec, w_im) == offsetof(fmr_iq_correction_record, w_im), "the fields of a record");
  cfg = m;
  coef.W = m.average_intervals; coef.R = m.record_intervals; coef.L = m.max_records; coef.act = m.mode == FMR_IQC_ACT;
  coef.dc = (m.correct & FMR_IQC_DC) != 0; coef.balance = (m.correct & FMR_IQC_BALANCE) != 0;
  int rc;
  if ((rc = CaptureStage::init(rows_, max_in, coef.act, m.record_intervals, m.max_records))) return rc;
  tring = 64;
  while (tring < pmax + m.average_intervals + 2) tring <<= 1;
  if ((rc = d_part.alloc((size_t)2 * rows * pmax))) return rc;
  if ((rc = d_tot.alloc((size_t)rows * tiles() * ((kIqcBack + 1) * kIqcCoefT + 1)))) return rc;
  if ((rc = d_tring.alloc((size_t)rows * tring))) return rc;
  if ((rc = d_state.alloc((size_t)rows))) return rc;
  if ((rc = d_ring.alloc((size_t)rows * (size_t)m.max_records))) return rc;
  if ((rc = ev_coef.create(hipEventDisableTiming))) return rc;
  on = true;
  return FMR_OK;
}

// One call's input rows (the samples [iqc.n, iqc.n + N_in) of every row at d_iq) through the corrector, in front of the
// blanker and of everything else that reads them; in FMR_IQC_ACT d_iq and stride then name the corrected rows.
int fmr_chain::iqc_stage(const float2 *&d_iq, size_t &stride, long long N_in) {
  IqCorrectionStage &b = iqc;
  CaptureStage::Call k;
  if (int rc = b.begin(k, "the IQ corrector", N_in, stream)) return rc;
  IqcPart *part = b.d_part.p + (size_t)k.par * b.rows * b.pmax;
  timed_on(stream, "iqc_moments", [&] {
    hipLaunchKernelGGL(k_iqc_moments, dim3((unsigned)k.pieces, b.rows), dim3(kNbT), 0, stream, d_iq, (long long)stride, k.n0, k.n1, b.pmax, part);
  });
  timed_on(stream, "iqc_coef", [&] {
    hipLaunchKernelGGL(k_iqc_coef, dim3((unsigned)((k.pieces + kIqcCoefT - 1) / kIqcCoefT), b.rows), dim3(kIqcCoefT), 0, stream, part, b.pmax, k.n0, k.n1, k.par, b.d_tot.p, b.d_tring.p,
                       b.tring - 1, b.d_state.p, b.coef);
  });
  HIPCHK(hipEventRecord(b.ev_coef, stream));
  b.out_rows(k, d_iq, stride);
  if (b.act)
    timed_on(stream, "iqc_apply", [&] {
      hipLaunchKernelGGL(k_iqc_apply, dim3((unsigned)k.pieces, b.rows), dim3(kNbT), 0, stream, d_iq, (long long)stride, k.out, k.ostride, k.n0, k.n1,
                         b.pmax, (const IqcPart *)part);
    });
  HIPCHK(hipStreamWaitEvent(side, b.ev_coef, 0));
  timed_on(side, "iqc_records", [&] {
    hipLaunchKernelGGL(k_iqc_records, dim3(b.rows), dim3(64), 0, side, (const IqcPart *)part, b.pmax, k.n0, k.n1, b.d_state.p, b.d_ring.p,
                       b.coef.R, b.coef.L);
  });
  return b.finish(k, side, d_iq, stride);
}

// ---- audio analyser (kernels_analyser.hpp) ----
template <int LOGN>
static void an_shape(AnalyserStage &a) {
  a.kseg = k_an_seg<LOGN>;
  a.threads = AnShape<LOGN>::T;
  a.lds = AnShape<LOGN>::LDS_BYTES;
}

int AnalyserStage::init(int S, size_t max_au, const fmr_analyser_config &m) {
  static_assert(sizeof(AnRec) == sizeof(fmr_analyser_record), "AnRec is fmr_analyser_record");
  static_assert(offsetof(fmr_analyser_record, sum) == offsetof(AnRec, sum), "the sums of a record");
  cfg = m;
  N = m.fft_size; H = N / 2; nb = N / 2 + 1;
  logn = 0;
  while ((1 << logn) < N) logn++;
  switch (logn) {
    case 10: an_shape<10>(*this); break;
    case 11: an_shape<11>(*this); break;
    case 12: an_shape<12>(*this); break;
    default: an_shape<13>(*this); break;
  }
  if (int rc = set_dyn_lds(kseg, (size_t)lds)) return rc;
  ws = welch_size((unsigned)H, m.interval_samples, max_au, 1, 16, 64, kAnMaxRuns);
  const WelchTables t = welch_tables(N, kWelchBlackmanHarris);
  sumw2 = t.sumw2;
  const size_t L = (size_t)m.max_records, rows = (size_t)S * ws.rmax, nb3 = (size_t)kAnRows * nb;
  int rc;
  if ((rc = upload_welch(t, d_win, d_tw))) return rc;
  if ((rc = alloc_all(d_carry, (size_t)S * N * 2, d_ppsd, rows * nb3, d_ppart, rows, d_open_psd, 2 * (size_t)S * nb3,
                      d_open_rec, 2 * (size_t)S, d_ring_psd, (size_t)S * L * nb3, d_ring_rec, (size_t)S * L)))
    return rc;
  cur.reset(S, m.max_records);
  on = true;
  return FMR_OK;
}

// one call's audio (N_au frames per stream, where the mux wrote them) through the analyser, on stream st
int fmr_chain::an_stage(const double *d_aud, long long astride, long long N_au, hipStream_t st) {
  if (N_au <= 0) return FMR_OK;
  AnArgs a{};
  a.ch = stereo ? 2 : 1;
  const int L = (int)an.cur.L, rmax = an.ws.rmax;
  const long long M = (long long)an.cfg.interval_samples;
  welch_call(an.ws, a, an.N, an.H, N_au,
    [&](int runs) {
      timed_on(st, "an_seg", [&] {
        hipLaunchKernelGGL(an.kseg, dim3(runs, S), dim3(an.threads), an.lds, st, d_aud, astride, an.d_carry.p, a, an.d_win.p,
                           an.d_tw.p, rmax, an.d_ppsd.p, an.d_ppart.p);
      });
    },
    [&](int runs, int nrec, long long n1, int last) {
      timed_on(st, "an_reduce", [&] {
        hipLaunchKernelGGL(k_an_reduce, dim3(nrec, S), dim3(kAnRT), 0, st, an.d_ppsd.p, an.d_ppart.p, runs, rmax, a, an.N, L, M,
                           an.ws.par, an.d_open_psd.p, an.d_open_rec.p, an.d_ring_psd.p, an.d_ring_rec.p, d_aud, astride,
                           an.d_carry.p, n1, last);
      });
    });
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- output stage (kernels_output.hpp) ----
int OutputStage::init(int S, bool chain_stereo, int max_blocks, int slots, const fmr_output_config &m) {
  static_assert(sizeof(OutRec) == sizeof(fmr_output_block), "OutRec is fmr_output_block");
  cfg = m;
  stereo = chain_stereo;
  ifrms_slot_len = (size_t)S * max_blocks;
  int rc;
  if ((rc = d_ifrms.alloc((size_t)slots * ifrms_slot_len))) return rc;
  if ((rc = d_part.alloc((size_t)S * max_blocks))) return rc;
  if ((rc = d_state.alloc((size_t)S))) return rc;
  if ((rc = d_rec.alloc((size_t)S * m.max_blocks))) return rc;
  if ((rc = d_pcm.alloc((size_t)S * m.max_frames * frame_bytes()))) return rc;
  fcur.reset(S, 1); fcur.L = m.max_frames;
  bcur.reset(S, (int)m.max_blocks);
  block = recs = frames = 0;
  on = true;
  return FMR_OK;
}

// the rate converter of an enabled stage, before the first block: the prototype, the two staging rows, the totals
int OutRate::init(int rate, bool to_mono, int S, bool stereo, size_t max_au) {
  std::vector<double> h;
  OutRateGeom gm{};
  if (!design_output_rate(rate, gm.L, gm.M, gm.T, &h)) { set_err("fmr_set_output_rate: rate %d has no design", rate); return FMR_ERR_BAD_ARG; }
  hz = rate; mono = to_mono; on = true;
  const int och = stereo && !mono ? 2 : 1;      // (OutputStage::channels with this converter)
  gm.span = (int)(((long long)(kOutThreads - 1) * gm.M) / gm.L) + 1 + gm.T;
  gm.zstride = ((long long)(gm.T - 1) + (long long)max_au) * och;
  gm.zrow = (long long)S * gm.zstride;
  geom = gm;
  int rc;
  if ((rc = d_taps.alloc(h.size()))) return rc;
  HIPCHK(hipMemcpy(d_taps.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  if ((rc = d_z.alloc((size_t)2 * gm.zrow))) return rc;      // (zeroed: z[j] = +0.0 for j < 0)
  if ((rc = d_tot.alloc((size_t)2 * S))) return rc;
  oframes = 0; zpar = 0;
  return FMR_OK;
}

// the positions of one call (block0: absolute index of its first block), taken when it is issued; advances the counters
OutArgs OutputStage::begin(unsigned long long block0, const int *if_len, int nb, long long N_au) {
  OutArgs a{};
  a.block0 = block0; a.frame0 = frames; a.rec0 = recs;
  a.n_frames = (unsigned long long)N_au;
  for (int b = 0; b < nb; b++) a.n_recs += if_len[b] != 0;
  a.squelch = cfg.squelch_level; a.gain = cfg.gain;
  a.max_frames = cfg.max_frames; a.max_blocks = cfg.max_blocks;
  frames += a.n_frames; recs += a.n_recs;
  if (rate.on) {      // ring frames: ceil(F L / M) after F decoder frames
    const unsigned long long L = (unsigned long long)rate.geom.L, M = (unsigned long long)rate.geom.M;
    a.out0 = rate.oframes;
    rate.oframes = (frames * L + M - 1) / M;
    a.n_out = rate.oframes - a.out0;
    a.zpar = rate.zpar;
    if (a.n_frames > 0) rate.zpar ^= 1;      // (a call without audio launches nothing: the history stays where it is)
  }
  return a;
}

// one call's audio (where the decoder wrote it) through the output stage on stream st: the PCM frames and the blocks'
// partials, then the records
int fmr_chain::out_stage(const double *d_aud, long long astride, const BlockTab &bt, const float *if_rms_blk, const OutArgs &a,
                         hipStream_t st) {
  if (a.n_recs == 0) return FMR_OK;
  const int ch = stereo ? 2 : 1;
  if (a.n_frames > 0)
    timed_on(st, "out_pcm", [&] {
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(bt.nb, S), dim3(kOutThreads), 0, st, d_aud, astride, bt, if_rms_blk, a,
                           out.rate.on ? (void *)nullptr : (void *)out.d_pcm.p, out.d_part.p);
      };
      if (out.cfg.format == FMR_PCM_F32) { if (ch == 2) go(k_out_pcm<1, 2>); else go(k_out_pcm<1, 1>); }
      else { if (ch == 2) go(k_out_pcm<0, 2>); else go(k_out_pcm<0, 1>); }
    });
  timed_on(st, "out_blocks", [&] {
    hipLaunchKernelGGL(k_out_blocks, dim3(S), dim3(64), 0, st, bt, if_rms_blk, (const OutPart *)out.d_part.p, a, ch, out.d_state.p,
                       out.d_rec.p);
  });
  if (out.rate.on && a.n_frames > 0) {
    const OutRateGeom &gm = out.rate.geom;
    const int och = out.channels();
    timed_on(st, "out_z", [&] {
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(bt.nb, S), dim3(kOutThreads), 0, st, d_aud, astride, bt, if_rms_blk, a, gm, out.rate.d_z.p);
      };
      if (ch == 1) go(k_out_z<1, 1>); else if (och == 2) go(k_out_z<2, 2>); else go(k_out_z<2, 1>);
    });
    if (a.n_out > 0)
      timed_on(st, "out_rate", [&] {
        const size_t lds = (size_t)gm.span * och * sizeof(double) + 2 * (kOutThreads / 64) * sizeof(unsigned);
        auto go = [&](auto kern) {
          hipLaunchKernelGGL(kern, dim3((unsigned)((a.n_out + kOutThreads - 1) / kOutThreads), S), dim3(kOutThreads), lds, st,
                             (const double *)out.rate.d_z.p, (const double *)out.rate.d_taps.p, gm, a, (void *)out.d_pcm.p, out.rate.d_tot.p);
        };
        if (out.cfg.format == FMR_PCM_F32) { if (och == 2) go(k_out_rate<1, 2>); else go(k_out_rate<1, 1>); }
        else { if (och == 2) go(k_out_rate<0, 2>); else go(k_out_rate<0, 1>); }
      });
    const int hist = (gm.T - 1) * och;
    if (hist > 0)
      timed_on(st, "out_hist", [&] {
        hipLaunchKernelGGL(k_out_hist, dim3((hist + kOutThreads - 1) / kOutThreads, S), dim3(kOutThreads), 0, st, out.rate.d_z.p, gm,
                           a.zpar, (long long)a.n_frames * och, hist);
      });
  }
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- MPX output (kernels_mpxout.hpp) ----
int MpxOutStage::init(int S, const fmr_mpx_output_config &m) {
  std::vector<double> h;
  MpxOutGeom gm{};
  if (!design_mpx_rate(m.rate, gm.L, gm.M, gm.T, &h)) { set_err("fmr_enable_mpx_output: rate %d has no design", m.rate); return FMR_ERR_BAD_ARG; }
  gm.span = (int)(((long long)(kMpxThreads - 1) * gm.M) / gm.L) + 1 + gm.T;
  cfg = m; geom = gm;
  int rc;
  if (gm.T > 1) {
    if ((rc = d_taps.alloc(h.size()))) return rc;
    HIPCHK(hipMemcpy(d_taps.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = d_carry.alloc((size_t)2 * S * (gm.T - 1)))) return rc;      // (zeroed: z[j] = +0.0 for j < 0)
  }
  if ((rc = d_tot.alloc((size_t)2 * S))) return rc;
  if ((rc = d_pcm.alloc((size_t)S * m.max_frames * frame_bytes()))) return rc;
  cur.reset(S, 1); cur.L = m.max_frames;
  n = oframes = 0; par = 0;
  on = true;
  return FMR_OK;
}

// the positions of one call, taken when it is issued; advances the counters
MpxOutArgs MpxOutStage::begin(long long N_if) {
  MpxOutArgs a{};
  const unsigned long long L = (unsigned long long)geom.L, M = (unsigned long long)geom.M;
  a.n0 = n; a.n = (unsigned long long)N_if;
  n += a.n;
  a.out0 = oframes;
  oframes = (n * L + M - 1) / M;      // ring frames: ceil(F L / M) after F MPX samples
  a.n_out = oframes - a.out0;
  a.gain = cfg.gain; a.max_frames = cfg.max_frames;
  a.par = par;
  if (a.n > 0) par ^= 1;      // (a call without MPX samples launches nothing: the carry stays where it is)
  return a;
}

// one call's MPX (the base slot of the call) through the MPX output on stream st
int fmr_chain::mpxout_stage(const fm_mpx_t *base, const MpxOutArgs &a, hipStream_t st) {
  if (a.n == 0) return FMR_OK;
  static_assert(sizeof(fm_mpx_t) == sizeof(float), "the MPX output reads the MPX as floats");
  const float *x = reinterpret_cast<const float *>(base);
  const long long bstride = H_b + (long long)max_if;
  const MpxOutGeom &gm = mpxo.geom;
  const bool f32 = mpxo.cfg.format == FMR_PCM_F32;
  if (gm.T == 1) {
    timed_on(st, "mpx_copy", [&] {
      hipLaunchKernelGGL(f32 ? k_mpx_copy<1> : k_mpx_copy<0>, dim3((unsigned)((a.n + kMpxThreads - 1) / kMpxThreads), S),
                         dim3(kMpxThreads), 0, st, x, bstride, H_b, a, (void *)mpxo.d_pcm.p, mpxo.d_tot.p);
    });
  } else {
    if (a.n_out > 0)
      timed_on(st, "mpx_rate", [&] {
        const size_t lds = (size_t)gm.span * sizeof(float) + 2 * (kMpxThreads / 64) * sizeof(unsigned);
        hipLaunchKernelGGL(f32 ? k_mpx_rate<1> : k_mpx_rate<0>, dim3((unsigned)((a.n_out + kMpxThreads - 1) / kMpxThreads), S),
                           dim3(kMpxThreads), lds, st, x, bstride, H_b, (const float *)mpxo.d_carry.p,
                           (const double *)mpxo.d_taps.p, gm, a, (void *)mpxo.d_pcm.p, mpxo.d_tot.p);
      });
    const int hist = gm.T - 1;
    timed_on(st, "mpx_hist", [&] {
      hipLaunchKernelGGL(k_mpx_hist, dim3((hist + kMpxThreads - 1) / kMpxThreads, S), dim3(kMpxThreads), 0, st, x, bstride, H_b,
                         mpxo.d_carry.p, hist, a);
    });
  }
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// ---- MPX input (kernels_mpxin.hpp) ----
int MpxInStage::init(int S, size_t max_in, int rate, int fmt, double gain_) {
  std::vector<double> h;
  MpxInGeom gm{1, 1, 1, 1, 0};
  if (!design_mpx_rate(rate, gm.L, gm.M, gm.T, &h)) { set_err("fmr_create_mpx_decoder: rate %d has no design", rate); return FMR_ERR_BAD_ARG; }
  gm.K = gm.T > 1 ? (int)(((long long)gm.T * gm.L + gm.M - 1) / gm.M) : 1;
  gm.span = (int)(((long long)(kMpxInThreads - 1) * gm.L) / gm.M) + 1 + gm.K;
  geom = gm; format = fmt; gain = gain_;
  g = gm.T > 1 ? gain_ * ((double)gm.M / (double)gm.L) : gain_;
  int rc;
  if (gm.T > 1) {
    std::vector<double> hp((size_t)gm.K * gm.M, 0.0);      // h[p + k M], zero from T L on
    std::copy(h.begin(), h.end(), hp.begin());
    if ((rc = upload(d_taps, hp.data(), hp.size()))) return rc;
    if (gm.K > 1 && (rc = d_carry.alloc((size_t)2 * S * (gm.K - 1)))) return rc;      // (zeroed: z[i] = +0.0 for i < 0)
  }
  if (fmt == FMR_PCM_S16) {
    std::vector<double> q(65536);
    for (int v = -32768; v <= 32767; v++) q[(size_t)(v + 32768)] = (double)v / 32767.0;
    if ((rc = upload(d_s16, q.data(), q.size()))) return rc;
  }
  if ((rc = d_tot.alloc((size_t)S))) return rc;
  if ((rc = d_pcm.alloc((size_t)S * max_in * frame_bytes()))) return rc;
  frames = samples = 0; par = 0;
  on = true;
  return FMR_OK;
}

// the positions of one call; advances the counters
MpxInArgs MpxInStage::begin(long long n_frames) {
  MpxInArgs a{};
  a.f0 = frames; a.nf = (unsigned long long)n_frames;
  frames += a.nf;
  a.j0 = samples;
  samples = samples_after(frames);
  a.n = samples - a.j0;
  a.g = g;
  a.par = par;
  if (a.nf > 0) par ^= 1;      // (a call without frames launches nothing: the carry stays where it is)
  return a;
}

// The front end of an MPX-input chain, where run_if_stage and k_disc stand on an IQ chain: the call's PCM rows to its MPX
// row and d_dec, the carry for the next call, then (behind the block table) the per-block baseband sums.
int fmr_chain::mpxin_stage(CallCtx &k) {
  const CallPlan &p = k.plan;
  k.xin = nullptr; k.x_stride = 0; k.x_off = 0; k.disc_gain = nullptr;
  k.agc_on_side = false; k.agc_deferred = false; agc_beside_mpf = false;
  if (!p.iter_on_side)      // (FMR_SERIAL=1: the round flags are reset here, as run_if_stage does it)
    hipLaunchKernelGGL(k_iter_begin, dim3(S), dim3(256), 0, stream, d_flags.p, (float *)nullptr, p.agc_nc, d_state.p, S,
                       (unsigned long long *)d_pll_sync.p, (int)(sizeof(PllSync) / 8), d_pll_tick2.p, pll_tick2_per_stream,
                       (unsigned int *)nullptr);
  const MpxInArgs a = mpxi.begin(k.N_in);
  if ((long long)a.n != k.N_if) { set_err("internal: the MPX input's count law and the block table disagree"); return FMR_ERR_HIP; }
  static_assert(sizeof(fm_mpx_t) == sizeof(float), "the MPX input writes the MPX as floats");
  float *x = reinterpret_cast<float *>(k.base);
  const long long bstride = H_b + (long long)max_if;
  const MpxInGeom &gm = mpxi.geom;
  const bool f32 = mpxi.format == FMR_PCM_F32;
  const void *pcm = k.d_iq;
  const long long pstride = (long long)k.stride;
  const dim3 grid((unsigned)((a.n + kMpxInThreads - 1) / kMpxInThreads), S);
  if (gm.T == 1) {
    timed("mpx_in_copy", [&] {
      hipLaunchKernelGGL(f32 ? k_mpx_in_copy<1> : k_mpx_in_copy<0>, grid, dim3(kMpxInThreads), 0, stream, pcm, pstride,
                         (const double *)mpxi.d_s16.p, a, x, bstride, H_b, d_dec.p, (long long)max_if, mpxi.d_tot.p);
    });
  } else {
    timed("mpx_in_rate", [&] {
      const size_t lds = (size_t)gm.span * sizeof(double) + (kMpxInThreads / 64) * sizeof(unsigned);
      hipLaunchKernelGGL(f32 ? k_mpx_in_rate<1> : k_mpx_in_rate<0>, grid, dim3(kMpxInThreads), lds, stream, pcm, pstride,
                         (const double *)mpxi.d_s16.p, (const double *)mpxi.d_carry.p, (const double *)mpxi.d_taps.p, gm, a, x, bstride, H_b, d_dec.p,
                         (long long)max_if, mpxi.d_tot.p);
    });
    const int hist = gm.K - 1;
    if (hist > 0)
      timed("mpx_in_hist", [&] {
        hipLaunchKernelGGL(f32 ? k_mpx_in_hist<1> : k_mpx_in_hist<0>, dim3((hist + kMpxInThreads - 1) / kMpxInThreads, S),
                           dim3(kMpxInThreads), 0, stream, pcm, pstride, (const double *)mpxi.d_s16.p, mpxi.d_carry.p, hist, a);
      });
  }
  timed("mpx_in_stats", [&] {      // (the decoder stream has waited for the block table: run_tables)
    hipLaunchKernelGGL(k_mpx_in_stats, dim3(k.nb, S), dim3(kMpxInThreads), 0, stream, (const float *)x, bstride, H_b, k.bt,
                       d_bb_mean_blk.p, d_bb_rms_blk.p, d_if_rms_blk.p);
  });
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// the filled slots, in call order, through the host decoders (never blocks)
void RdsStage::drain() {
  while (drained < seq && __atomic_load_n(h_mark.p, __ATOMIC_ACQUIRE) > drained) {
    const unsigned long long q = ++drained;
    const char *slot = h_slots.p + (size_t)(q % kSlots) * S * slot_stride;
    for (int s = 0; s < S; s++) {
      const char *sl = slot + (size_t)s * slot_stride;
      RdsSlotHdr h;
      memcpy(&h, sl, sizeof h);
      const RdsRec *rec = reinterpret_cast<const RdsRec *>(sl + sizeof(RdsSlotHdr));
      const unsigned char *bits = reinterpret_cast<const unsigned char *>(sl + rds_slot_bits_off(maxw));
      const float *rho = reinterpret_cast<const float *>(sl + rds_slot_rho_off(maxw));
      for (int w = 0; w < h.nw && w < maxw; w++) {
        const RdsRec r = rec[w];
        const float *rw = rho + (size_t)w * (kRdsMaxSym + 1);
        if (r.count > 0) dec[s].carried(rw[0]);
        for (int t = 0; t < r.count && t < kRdsMaxSym; t++) {
          const long long pos = (r.k_first + t) * kRdsSym + r.tau;       // [U]
          dec[s].push(bits[(size_t)w * kRdsMaxSym + t], pos > 0 ? (uint64_t)((pos + 9) / 19) : 0, rw[t + 1]);
        }
      }
      hdr[s] = h;
    }
  }
}

// Pipelined chain: enqueue the tail stage of the last decoded call on the tail stream, behind `gate` (the front end of
// the call that follows it; null: nothing to wait for but the call's own PLL stage).
int fmr_chain::flush_walk() {
  if (!walk_pending) return FMR_OK;
  walk_pending = false;
  return pll_walk(walk_job);
}
int fmr_chain::flush_tail(hipEvent_t gate) {
  const int rc_walk = flush_walk();       // (the tail's output mux waits for its call's walk: enqueued first, or the wait finds an older record)
  if (rc_walk != FMR_OK && !tail_pending) return rc_walk;
  if (!tail_pending) return FMR_OK;
  tail_pending = false;
  const int rc = enqueue_tail(gate);
  if (rc != FMR_OK)      // the slot of the ring must still be released, or the calls that reuse it wait for a mark that never comes
    hipLaunchKernelGGL(k_signal_host, dim3(1), dim3(1), 0, tail, &h_marks.p[1], tail_job.seq);
  return rc != FMR_OK ? rc : rc_walk;     // (a walk that could not be enqueued leaves that call's lock flags and PPS events stale: an error of this call)
}
int fmr_chain::enqueue_tail(hipEvent_t gate) {
  TailCtx t = tail_job;
  if (!gate && t.can_split && !t.mono_enqueued && t.ev_mpx) {
    // Drain (a synchronising call, no front end follows): the mono channel does not depend on the PLL -- it starts from the
    // MPX, behind the tail of the call before (same stream, enqueued when this call's front end was), beside this call's
    // PLL passes.  A caller that synchronises after every call gets its audio 0.1 ms earlier; a timed region of K calls
    // ends that much earlier.  (In steady state the tail waits for the NEXT front end instead: see run_fm.)
    HIPCHK(hipStreamWaitEvent(tail, t.ev_mpx, 0));
    tail_channels(t, tail, 0, 1);
    HIPCHK(hipEventRecord(ev_mono, tail));
    t.mono_enqueued = true;
  }
  HIPCHK(hipStreamWaitEvent(tail, ev_pll, 0));
  if (gate) HIPCHK(hipStreamWaitEvent(tail, gate, 0));
#ifndef FMR_DIAG_NO_TAIL      // (diagnostic builds under tools/: what the step costs without the tail's kernels beside the next front end)
  if (int rc = tail_stage(t, tail)) return rc;
#endif
  if (t.ht.n) {
    timed_on(tail, "shift_halo", [&] { hipLaunchKernelGGL(k_shift_halo<256>, dim3(t.ht.n, S), dim3(256), 0, tail, t.ht); });
  }
  hipLaunchKernelGGL(k_signal_host, dim3(1), dim3(1), 0, tail, &h_marks.p[1], t.seq);
  HIPCHK(hipGetLastError());
  return FMR_OK;
}

// NbfmDecoder
int fmr_chain::run_nbfm(CallCtx &k) {
  const int nb = k.nb;
  const long long N_if = k.N_if, astride = (long long)k.astride;
  const BlockTab &bt = k.bt; double *const d_aud = k.d_aud;
  // NbfmDecoder (NbfmDecode.cpp:47-96): discriminator on the AGC'd IF, statistics, 63-tap audio FIR (same
  // block-head path as the FM pilot cut: LowPassFilterFirAudio), -3 dB.  No resampling: audio block = IF block.
  const long long base_stride = H_b + (long long)max_if;
  timed("disc", [&] {
    hipLaunchKernelGGL((k_disc<256, double>), dim3(nb, S), dim3(256), 0, stream, k.xin, k.x_stride, k.x_off, d_gain.p,
                       (long long)max_if, (float2 *)nullptr, (long long)max_if, d_mpf_ok.p, bt, disc_nf, disc_bound,
                       d_dec.p, (long long)max_if, d_base.p, base_stride, H_b, d_bb_mean_blk.p, d_bb_rms_blk.p,
                       d_state.p, (float *)nullptr);
  });
  timed("stats", [&] {
    hipLaunchKernelGGL(k_stats, dim3(S), dim3(FMR_STATS_THREADS), 0, stream, bt, d_if_rms_blk.p, d_bb_mean_blk.p,
                       d_bb_rms_blk.p, d_state.p, S, 1, (const FusedPart *)nullptr, 0, 0, out.ifrms_slot(0), 1);
  });
  timed("nbfm_audio", [&] {
    hipLaunchKernelGGL((k_pilotcut2<320, 1280>), dim3(nb, S, 1), dim3(320), 0, stream, d_base.p, (double *)nullptr,
                       base_stride, H_b, bt, d_pilotcut.p, n_pilotcut, d_aud, (double *)nullptr, astride,
                       0.70794578438413791, 0);       // std::pow(10.0, -3.0 / 20.0), NbfmDecode.cpp:91
  });
  k.add_halo(k.ifbuf, k.if_stride, H_if, N_if);
  k.add_halo(d_base.p, base_stride, H_b, N_if);
  if (k.audio_len) for (int b = 0; b < nb; b++) k.audio_len[b] = (uint32_t)k.tab.au_len[b];
  if (an.on) if (int rc = an_stage(d_aud, astride, k.N_au, stream)) return rc;
  if (out.on) if (int rc = out_stage(d_aud, astride, bt, out.ifrms_slot(0), out.begin(k.out_block0, k.tab.if_len, nb, k.N_au), stream)) return rc;
  return FMR_OK;
}

// AmDecoder (AM / DSB / USB / LSB / CW / WSPR)
int fmr_chain::run_am(CallCtx &k) {
  const int nb = k.nb;
  const long long N_if = k.N_if, astride = (long long)k.astride;
  const BlockTab &bt = k.bt; double *const d_aud = k.d_aud;
  timed("am_demod", [&] {
    hipLaunchKernelGGL(k_am_demod<256>, dim3(nb, S), dim3(256), 0, stream, k.xin, k.x_stride, k.x_off, d_gain.p,
                       (long long)max_if, bt, (int)(mode != FMR_MODE_AM), d_dec.p, (long long)max_if, d_base.p,
                       (long long)max_if, d_bb_mean_blk.p, d_bb_rms_blk.p);
  });
  timed("stats", [&] {
    hipLaunchKernelGGL(k_stats, dim3(S), dim3(FMR_STATS_THREADS), 0, stream, bt, d_if_rms_blk.p, d_bb_mean_blk.p,
                       d_bb_rms_blk.p, d_state.p, S, 0, (const FusedPart *)nullptr, 0, 0, out.ifrms_slot(0));
  });
  timed("am_tail", [&] {
    const bool par_tail = !env.serial;
    if (par_tail) {
      // DC block -> AfSimpleAgc -> de-emphasis in time-parallel form (kernels_par.hpp); the serial kernel below only
      // runs for a stream whose Newton rounds did not converge
      const int nc = (int)((N_if + C_AM - 1) / C_AM);
      const AfAgcCoef af{1.0, 1.5, af_ref, af_rate};      // AfSimpleAgc(1.0, 1.5, reference, rate): AmDecode.cpp:54-66
      hipLaunchKernelGGL(k_dc_pass1<C_AM>, dim3((nc + 63) / 64, S, 1), dim3(64), 0, stream, d_base.p, (const double *)nullptr,
                         (long long)max_if, (int)N_if, am_dk, d_dc_G.p, nc, 0);
      const int dc_nw = std::max(1, std::min(FMR_DC_MAXW, (nc + 64 * FMR_DC_K - 1) / (64 * FMR_DC_K)));
      hipLaunchKernelGGL(k_dc_nodes, dim3(S), dim3(64 * dc_nw), 0, stream, d_dc_G.p, d_dc_start.p, nc, am_dk, d_state.p, S, 0);
      hipLaunchKernelGGL(k_af_begin, dim3(S), dim3(256), 0, stream, d_flags.p, d_af_nodes.p, nc, d_state.p, d_af_tick.p);
      for (int it = 0; it < K_AF_ITERS; it++)
        hipLaunchKernelGGL(k_af_round<C_AM>, dim3((nc + 63) / 64, S), dim3(64), 0, stream, d_base.p, (long long)max_if, (int)N_if,
                           am_dk, d_dc_start.p, af, d_af_nodes.p, d_af_G.p, d_af_M.p, d_af_out.p, (long long)max_if, nc,
                           d_state.p, d_flags.p, d_af_tick.p);
      const int ncd = (int)((N_if + C_AM_DE - 1) / C_AM_DE);
      hipLaunchKernelGGL(k_am_deemph_out<C_AM_DE>, dim3((ncd + 63) / 64, S), dim3(64), 0, stream, d_af_out.p, (long long)max_if,
                         (int)N_if, am_deemph.b0, am_deemph.a1, (int)(mode == FMR_MODE_AM), d_aud, astride,
                         d_state.p, d_flags.p);
      hipLaunchKernelGGL(k_am_commit, dim3((S + 63) / 64), dim3(64), 0, stream, d_state.p, d_flags.p, S);
    }
    hipLaunchKernelGGL(k_am_tail, dim3((S + 63) / 64), dim3(64), 0, stream, d_base.p, (long long)max_if, (int)N_if,
                       am_dcblock.b0, am_dcblock.b1, am_dcblock.b2, am_dcblock.a1, am_dcblock.a2, 1.0, 1.5, af_ref,
                       af_rate, am_deemph.b0, am_deemph.a1, (int)(mode == FMR_MODE_AM), d_aud, astride,
                       d_state.p, S, par_tail ? &d_flags.p->af_converged : (const int *)nullptr, (int)sizeof(IterFlags),
                       par_tail ? &d_flags.p->af_fallback : (int *)nullptr);
  });
  k.add_halo(k.ifbuf, k.if_stride, H_if, N_if);
  if (k.audio_len) for (int b = 0; b < nb; b++) k.audio_len[b] = (uint32_t)k.tab.au_len[b];
  if (an.on) if (int rc = an_stage(d_aud, astride, k.N_au, stream)) return rc;
  if (out.on) if (int rc = out_stage(d_aud, astride, bt, out.ifrms_slot(0), out.begin(k.out_block0, k.tab.if_len, nb, k.N_au), stream)) return rc;
  return FMR_OK;
}

// ============================================================================
// Band spectrum (fmr_spectrum_*, kernels_spectrum.hpp)
// ============================================================================
struct fmr_spectrum {
  fmr_spectrum_config cfg{};
  int N = 0, H = 0, logn = 0, rows = 0, fmt = 0;
  int rmax = 1;                          // runs per row and call (capacity of the partials)
  int n_cu = 256;
  Stream stream;
  DevBuf<float> d_win, d_pmax, d_max;
  DevBuf<float2> d_tw, d_ring;
  DevBuf<double> d_psum, d_sum;
  DevBuf<int2> d_pcnt;
  DevBuf<unsigned long long> d_cnt;      // per row: segments counted, segments skipped
  DevBuf<unsigned char> d_stage;         // host path: the call's rows
  unsigned long long total = 0;          // samples per row since create
  unsigned long long next_seg = 0;       // segments completed since create
  unsigned long long first_seg = 0;      // first segment processed since create / the last reset
  double sumw = 0.0, sumw2 = 0.0;
  // waterfall (fmr_spectrum_create_waterfall; wf.segments_per_line = 0: none)
  fmr_waterfall_config wf{};
  int wf_sb = 0, wf_par = 0;             // sub-blocks per line; which copy of the open line's partial is current
  DevBuf<float> d_plsub, d_wopen, d_wline, d_wring;
  DevBuf<int> d_plcnt, d_wopen_cnt, d_wline_cnt;
  DevBuf<unsigned> d_wring_cnt;
  RecCursor wf_cur;                      // per row: next unread line, lines overwritten unread
  int init();
  int run(const void *d_in, size_t stride, size_t n);
  int run_waterfall(const void *d_in, size_t stride, long long tb, long long ta, long long j_hi);
  ~fmr_spectrum() { if (stream) (void)hipStreamSynchronize(stream); }      // (the stream idle, then the members: as ~fmr_chain)
};

namespace {
constexpr int kSpecBps[4] = {8, 4, 2, 2};    // bytes per IQ sample of FMR_IQ_CF32 / S16 / U8 / S8
// limits of fmr_spectrum_create: grid.y is 65535 rows at most; a call of 2^30 samples per row has at most 2^30 segments
// (H = 1), so every segment count and index k_spec_seg and the engine hold in int stays below 2^31
constexpr int kSpecMaxRows = 65535;
constexpr size_t kSpecMaxCall = (size_t)1 << 30;

// wf = nullptr: the plain form; else the waterfall form with these arguments
template <int LOGN, int FMT>
int spec_seg_launch(fmr_spectrum *s, dim3 grid, const void *in, long long stride, long long tb, long long seg0, int n_seg,
                    int per_run, const SpecWf *wf) {
  if (wf)
    hipLaunchKernelGGL((k_spec_seg<LOGN, FMT, true>), grid, dim3(SpecShape<LOGN>::T), SpecShape<LOGN>::LDS_BYTES, s->stream, in,
                       stride, (const float2 *)s->d_ring.p, tb, seg0, n_seg, per_run, s->H, (const float *)s->d_win.p,
                       (const float2 *)s->d_tw.p, s->d_psum.p, s->d_pmax.p, s->d_pcnt.p, s->rmax, *wf);
  else
    hipLaunchKernelGGL((k_spec_seg<LOGN, FMT, false>), grid, dim3(SpecShape<LOGN>::T), SpecShape<LOGN>::LDS_BYTES, s->stream, in,
                       stride, (const float2 *)s->d_ring.p, tb, seg0, n_seg, per_run, s->H, (const float *)s->d_win.p,
                       (const float2 *)s->d_tw.p, s->d_psum.p, s->d_pmax.p, s->d_pcnt.p, s->rmax, SpecWf{});
  HIPCHK(hipGetLastError());
  return FMR_OK;
}
template <int LOGN, int FMT>
int spec_seg_attr(bool wf) {
  const void *fn = wf ? reinterpret_cast<const void *>(&k_spec_seg<LOGN, FMT, true>)
                      : reinterpret_cast<const void *>(&k_spec_seg<LOGN, FMT, false>);
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, SpecShape<LOGN>::LDS_BYTES));
  return FMR_OK;
}
using SpecSegFn = int (*)(fmr_spectrum *, dim3, const void *, long long, long long, long long, int, int, const SpecWf *);
using SpecAttrFn = int (*)(bool);
#define FMR_SPEC_ROW(L) {&spec_seg_launch<L, 0>, &spec_seg_launch<L, 1>, &spec_seg_launch<L, 2>, &spec_seg_launch<L, 3>}
#define FMR_SPEC_ATTR(L) {&spec_seg_attr<L, 0>, &spec_seg_attr<L, 1>, &spec_seg_attr<L, 2>, &spec_seg_attr<L, 3>}
const SpecSegFn kSpecSeg[7][4] = {FMR_SPEC_ROW(8), FMR_SPEC_ROW(9), FMR_SPEC_ROW(10), FMR_SPEC_ROW(11), FMR_SPEC_ROW(12),
                                  FMR_SPEC_ROW(13), FMR_SPEC_ROW(14)};
const SpecAttrFn kSpecAttr[7][4] = {FMR_SPEC_ATTR(8), FMR_SPEC_ATTR(9), FMR_SPEC_ATTR(10), FMR_SPEC_ATTR(11), FMR_SPEC_ATTR(12),
                                    FMR_SPEC_ATTR(13), FMR_SPEC_ATTR(14)};
#undef FMR_SPEC_ROW
#undef FMR_SPEC_ATTR
const decltype(&k_spec_reduce<0>) kSpecReduce[4] = {&k_spec_reduce<0>, &k_spec_reduce<1>, &k_spec_reduce<2>, &k_spec_reduce<3>};


// the rules of fmr_spectrum_create, before the device is opened
int spec_check(const fmr_spectrum_config &c) {
  if (c.fft_size < 256 || c.fft_size > 16384 || (c.fft_size & (c.fft_size - 1)) != 0) {
    set_err("fmr_spectrum_create: fft_size %d is not a power of two in 256 .. 16384", c.fft_size);
    return FMR_ERR_BAD_ARG;
  }
  if (c.hop < 0 || c.hop > c.fft_size) { set_err("fmr_spectrum_create: hop %d is outside 0 .. fft_size (%d)", c.hop, c.fft_size); return FMR_ERR_BAD_ARG; }
  if (c.window < FMR_WINDOW_HANN || c.window > FMR_WINDOW_BLACKMAN_HARRIS) { set_err("fmr_spectrum_create: unknown window %d", c.window); return FMR_ERR_BAD_ARG; }
  if (c.input_format < FMR_IQ_CF32 || c.input_format > FMR_IQ_S8) { set_err("fmr_spectrum_create: unknown input_format %d", c.input_format); return FMR_ERR_BAD_ARG; }
  if (!(c.input_rate > 0.0) || !std::isfinite(c.input_rate)) { set_err("fmr_spectrum_create: input_rate %g is not > 0", c.input_rate); return FMR_ERR_BAD_ARG; }
  if (c.n_rows < 1 || c.n_rows > kSpecMaxRows) {
    set_err("fmr_spectrum_create: n_rows %d is outside 1 .. %d (one grid row per IQ row)", c.n_rows, kSpecMaxRows);
    return FMR_ERR_BAD_ARG;
  }
  if (c.max_call_len == 0 || c.max_call_len > kSpecMaxCall) {
    set_err("fmr_spectrum_create: max_call_len %zu is outside 1 .. %zu (segments per call are counted in int)", c.max_call_len, kSpecMaxCall);
    return FMR_ERR_BAD_ARG;
  }
  return FMR_OK;
}

// the rules of fmr_spectrum_create_waterfall for the waterfall's own fields, before the device is opened
constexpr size_t kWfMaxBytes = (size_t)1 << 30;
int wf_check(const fmr_spectrum_config &c, const fmr_waterfall_config &w) {
  if (w.segments_per_line < 1 || w.segments_per_line > 65536) {
    set_err("fmr_spectrum_create_waterfall: segments_per_line %d is outside 1 .. 65536", w.segments_per_line);
    return FMR_ERR_BAD_ARG;
  }
  if (w.max_lines < 1) { set_err("fmr_spectrum_create_waterfall: max_lines %d is < 1", w.max_lines); return FMR_ERR_BAD_ARG; }
  if (w.which != FMR_WATERFALL_MEAN && w.which != FMR_WATERFALL_PEAK) {
    set_err("fmr_spectrum_create_waterfall: unknown which %d", w.which);
    return FMR_ERR_BAD_ARG;
  }
  if ((size_t)w.max_lines > kWfMaxBytes / 4 / (size_t)c.fft_size / (size_t)c.n_rows) {
    set_err("fmr_spectrum_create_waterfall: max_lines %d: n_rows (%d) x max_lines x fft_size (%d) x 4 bytes is above 1 GiB",
            w.max_lines, c.n_rows, c.fft_size);
    return FMR_ERR_BAD_ARG;
  }
  return FMR_OK;
}

// fmr_spectrum_config as the caller knows it -> this library's; then spec_check
int spec_take_cfg(const fmr_spectrum_config *cfg, size_t cfg_size, fmr_spectrum_config &full) {
  if (int rc = take_sized("fmr_spectrum_create", "fmr_spectrum_config", cfg, cfg_size, full)) return rc;
  return spec_check(full);
}
}  // namespace

int fmr_spectrum::init() {
  N = cfg.fft_size;
  H = cfg.hop ? cfg.hop : N / 2;
  logn = 0;
  while ((1 << logn) < N) logn++;
  rows = cfg.n_rows;
  fmt = cfg.input_format;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device"); return FMR_ERR_NO_DEVICE; }
  if (cfg.device < 0 || cfg.device >= ndev) { set_err("fmr_spectrum_create: device %d out of range (%d devices)", cfg.device, ndev); return FMR_ERR_BAD_ARG; }
  HIPCHK(hipSetDevice(cfg.device));
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg.device) == hipSuccess && prop.multiProcessorCount > 0) n_cu = prop.multiProcessorCount;
  if (int rc = stream.create()) return rc;
  const bool wfon = wf.segments_per_line > 0;
  if (int rc = kSpecAttr[logn - 8][fmt](wfon)) return rc;
  const WelchTables t = welch_tables(N, cfg.window);
  sumw = t.sumw;
  sumw2 = t.sumw2;
  if (int rc = upload_welch(t, d_win, d_tw)) return rc;
  // runs: about one workgroup per slot the chip holds at this N, shared by the rows; no more than a call's segments
  const int occ = std::max(1, std::min(163840 / spec_lds_bytes(logn), 2048 / spec_threads(logn)));
  const long long smax = (long long)((cfg.max_call_len + H - 1) / H) + 1;
  rmax = (int)std::max(1LL, std::min(smax, (long long)((n_cu * occ + rows - 1) / rows)));
  if (wfon) {
    // waterfall runs hold SPEC_WF_SUB segments at most, so a call is taken in launches of rmax runs per row: room for
    // more runs than the chip holds at once (up to 128 MiB of partials, 16 N bytes per run) keeps the launches few
    wf_sb = (wf.segments_per_line + SPEC_WF_SUB - 1) / SPEC_WF_SUB;
    const long long room = ((long long)128 << 20) / ((long long)rows * N * 16);
    rmax = (int)std::max<long long>(rmax, std::min(smax, room));
  }
  const size_t part = (size_t)rows * rmax;
  if (int rc = d_psum.alloc(part * N)) return rc;
  if (int rc = d_pmax.alloc(part * N)) return rc;
  if (int rc = d_pcnt.alloc(part)) return rc;
  if (int rc = d_sum.alloc((size_t)rows * N)) return rc;
  if (int rc = d_max.alloc((size_t)rows * N)) return rc;
  if (int rc = d_ring.alloc((size_t)rows * N)) return rc;
  if (int rc = d_cnt.alloc((size_t)rows * 2)) return rc;
  if (wfon) {
    if (int rc = d_plsub.alloc(part * N)) return rc;
    if (int rc = d_plcnt.alloc(part)) return rc;
    if (int rc = d_wopen.alloc((size_t)rows * N)) return rc;
    if (int rc = d_wopen_cnt.alloc(rows)) return rc;
    if (int rc = d_wline.alloc((size_t)2 * rows * N)) return rc;
    if (int rc = d_wline_cnt.alloc((size_t)2 * rows)) return rc;
    if (int rc = d_wring.alloc((size_t)rows * wf.max_lines * N)) return rc;
    if (int rc = d_wring_cnt.alloc((size_t)rows * wf.max_lines)) return rc;
    wf_cur.reset(rows, wf.max_lines);
  }
  HIPCHK(hipDeviceSynchronize());
  return FMR_OK;
}

// one call: n samples of every row at d_in (row r at d_in + r stride samples), on the object's stream
int fmr_spectrum::run(const void *d_in, size_t stride, size_t n) {
  const long long tb = (long long)total, ta = tb + (long long)n;
  const long long j_hi = ta >= N ? (ta - N) / H + 1 : 0;
  const long long n_seg = std::max(0LL, j_hi - (long long)next_seg);
  if (wf.segments_per_line > 0 && n_seg > 0) return run_waterfall(d_in, stride, tb, ta, j_hi);
  int runs = 0;
  if (n_seg > 0) {
    runs = (int)std::min<long long>(n_seg, rmax);
    const int per_run = (int)((n_seg + runs - 1) / runs);
    runs = (int)((n_seg + per_run - 1) / per_run);
    if (int rc = kSpecSeg[logn - 8][fmt](this, dim3(runs, rows), d_in, (long long)stride, tb, (long long)next_seg, (int)n_seg, per_run, nullptr))
      return rc;
  }
  hipLaunchKernelGGL(kSpecReduce[fmt], dim3((N + 63) / 64, rows), dim3(64 * SPEC_RW), 0, stream, (const double *)d_psum.p,
                     (const float *)d_pmax.p, (const int2 *)d_pcnt.p, runs, rmax, N, d_sum.p, d_max.p, d_cnt.p, d_in,
                     (long long)stride, tb, ta, d_ring.p);
  HIPCHK(hipGetLastError());
  if (n_seg > 0) next_seg = (unsigned long long)j_hi;
  total = (unsigned long long)ta;
  return FMR_OK;
}

// The call's segments [next_seg, j_hi) with the waterfall on: launches of at most rmax runs per row, run r of a launch =
// sub-block g0 + r of the line grid clipped to the launch (kernels_spectrum.hpp), each followed by the reduction of its
// partials (the sample ring is refreshed by the last one only: the launches before it still read it) and by the lines.
int fmr_spectrum::run_waterfall(const void *d_in, size_t stride, long long tb, long long ta, long long j_hi) {
  const int R = wf.segments_per_line;
  long long a = (long long)next_seg;
  while (a < j_hi) {
    const WelchLaunch p = welch_plan(R, SPEC_WF_SUB, wf_sb, rmax, a, j_hi);
    const int runs = p.runs;
    SpecWf w{};
    w.which = wf.which; w.R = R; w.SB = wf_sb; w.g0 = p.g0; w.a1 = p.a1;
    w.plsub = d_plsub.p; w.plcnt = d_plcnt.p; w.open_sub = d_wopen.p; w.open_cnt = d_wopen_cnt.p;
    if (int rc = kSpecSeg[logn - 8][fmt](this, dim3(runs, rows), d_in, (long long)stride, tb, a, (int)(w.a1 - a), 0, &w))
      return rc;
    hipLaunchKernelGGL(kSpecReduce[fmt], dim3((N + 63) / 64, rows), dim3(64 * SPEC_RW), 0, stream, (const double *)d_psum.p,
                       (const float *)d_pmax.p, (const int2 *)d_pcnt.p, runs, rmax, N, d_sum.p, d_max.p, d_cnt.p, d_in,
                       (long long)stride, tb, w.a1 == j_hi ? ta : tb, d_ring.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_spec_lines, dim3((unsigned)p.nrec, rows, (N + 255) / 256), dim3(256), 0, stream, w, a, runs,
                       rmax, N, wf.max_lines, wf_par, d_wline.p, d_wline_cnt.p, d_wring.p, d_wring_cnt.p);
    HIPCHK(hipGetLastError());
    wf_par ^= 1;
    a = w.a1;
  }
  next_seg = (unsigned long long)j_hi;
  total = (unsigned long long)ta;
  return FMR_OK;
}

static int spectrum_call(fmr_spectrum *s, const void *iq, size_t row_stride, size_t n, bool host, int sync) {
  if (!s || (!iq && n > 0)) { set_err("fmr_spectrum_process: null argument"); return FMR_ERR_BAD_ARG; }
  if (n > s->cfg.max_call_len) {
    set_err("fmr_spectrum_process: n = %zu > max_call_len = %zu (nothing was processed)", n, s->cfg.max_call_len);
    return FMR_ERR_CAPACITY;
  }
  if (row_stride == 0) row_stride = n;
  if (row_stride < n) { set_err("fmr_spectrum_process: row_stride %zu < n %zu", row_stride, n); return FMR_ERR_BAD_ARG; }
  if (n == 0) return FMR_OK;
  try {
    HIPCHK(hipSetDevice(s->cfg.device));
    const size_t bps = kSpecBps[s->fmt];
    const void *d_in = iq;
    size_t stride = row_stride;
    if (host) {
      const size_t need = (size_t)s->rows * s->cfg.max_call_len * bps;
      if (!s->d_stage.p) {
        if (s->d_stage.alloc(need)) return FMR_ERR_HIP;
        HIPCHK(hipDeviceSynchronize());      // (alloc's memset runs on the null stream, which the object's stream does not wait for)
      }
      HIPCHK(hipMemcpy2DAsync(s->d_stage.p, n * bps, iq, row_stride * bps, n * bps, s->rows, hipMemcpyHostToDevice, s->stream));
      d_in = s->d_stage.p;
      stride = n;
    }
    if (int rc = s->run(d_in, stride, n)) return rc;
    if (host || sync) HIPCHK(hipStreamSynchronize(s->stream));
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

// 10 log10 of a power ratio
static double spec_db(double x) { return 10.0 * std::log10(x); }

// The body of every fmr_*_read of a record ring.  `which` is the stage in the chain, `noun` and `enable` name it and its
// fmr_enable_*; idx is a stream of the chain, or an input row of a capture stage.  Refuses bad arguments and a chain
// without the stage, synchronises, then drains up to cap records of idx, oldest first: copy(st, k, at, m) fetches records
// k .. k + m of the read from the ring positions at .. at + m (at = idx L + slot) and returns FMR_OK or an error;
// scale(st, n), where given, turns what was drained into what the caller gets; fill(full, st) sets the stage's own fields
// of the info, whose struct_size and reader's view (ring_info) are set here.  Returns the count (cap = 0: the number
// waiting, nothing drained) or an error code.
template <class Stage, class Rec, class Info, class Copy, class Scale, class Fill>
static int read_records(const char *fn, fmr_chain *c, Stage fmr_chain::*which, const char *noun, const char *enable, int idx,
                        Rec *recs, int cap, Info *info, size_t info_size, Copy &&copy, Scale &&scale, Fill &&fill) {
  constexpr bool by_row = std::is_base_of_v<CaptureStage, Stage>;
  if (!c || cap < 0 || (!by_row && (idx < 0 || idx >= c->S))) {
    set_err(by_row ? "%s: bad chain or cap" : "%s: bad chain, stream or cap", fn);
    return FMR_ERR_BAD_ARG;
  }
  Stage &st = c->*which;
  if (!st.on) { set_err("%s: the chain has no %s (%s)", fn, noun, enable); return FMR_ERR_BAD_ARG; }
  if constexpr (by_row)
    if (idx < 0 || idx >= st.rows) { set_err("%s: row %d is not one of the chain's %d input rows", fn, idx, st.rows); return FMR_ERR_BAD_ARG; }
  if (cap > 0 && !recs) { set_err("%s: recs is null", fn); return FMR_ERR_BAD_ARG; }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    const unsigned long long done = st.done();
    const int n = st.cur.take(idx, done, (unsigned long long)cap, [&](size_t k, size_t slot, size_t m) -> int {
      return copy(st, k, (size_t)idx * (size_t)st.cur.L + slot, m);
    });
    if (n < 0) return n;
    if constexpr (!std::is_null_pointer_v<std::decay_t<Scale>>) scale(st, n);
    if (info) {
      Info full{};
      full.struct_size = (unsigned)sizeof full;
      ring_info(full, st.cur, idx, done);
      fill(full, st);
      give_sized(info, info_size, full);
    }
    return n;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

// copy() of a stage whose records lie in one ring, d_ring, as the caller gets them
template <class Rec>
static auto copy_ring(Rec *recs) {
  return [recs](auto &st, size_t k, size_t at, size_t m) -> int {
    static_assert(sizeof *st.d_ring.p == sizeof(Rec), "the ring holds the caller's records");
    HIPCHK(hipMemcpy(recs + k, st.d_ring.p + at, m * sizeof(Rec), hipMemcpyDeviceToHost));
    return FMR_OK;
  };
}

// copy() of the modulation monitor and the RF monitor (Rec = either record, which MonRec is): records, histograms and
// the PSD sums scaled to densities
template <class Rec>
static auto copy_seg_monitor(Rec *recs, uint32_t *hist, double *psd) {
  return [=](SegMonitor &m, size_t k0, size_t at, size_t nr) -> int {
    const size_t B = (size_t)m.bins;
    const double scale = 1.0 / (kFmRate * m.sumw2);
    HIPCHK(hipMemcpy(recs + k0, m.d_ring_rec.p + at, nr * sizeof(Rec), hipMemcpyDeviceToHost));
    if (hist) HIPCHK(hipMemcpy(hist + k0 * B, m.d_ring_hist.p + at * B, nr * B * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!psd) return FMR_OK;
    HIPCHK(hipMemcpy(psd + k0 * kMonPsd, m.d_ring_psd.p + at * kMonPsd, nr * kMonPsd * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t k = k0; k < k0 + nr; k++) {
      const double cnt = (double)recs[k].segments;
      double *p = psd + k * kMonPsd;
      for (int i = 0; i < kMonPsd; i++)
        p[i] = recs[k].segments == 0 ? 0.0 : p[i] / cnt * ((i == 0 || i == kMonPsd - 1) ? 1.0 : 2.0) * scale;
    }
    return FMR_OK;
  };
}

// A field of an fmr_enable_* configuration that has a default for 0 and a closed range: fills the default, refuses the rest
template <class T>
static int check_field(const char *fn, const char *name, T &x, long long lo, long long hi, long long dflt) {
  if (x == 0) x = (T)dflt;
  if ((long long)x >= lo && (long long)x <= hi) return FMR_OK;
  set_err("%s: %s %lld is outside %lld .. %lld (0 = %lld)", fn, name, (long long)x, lo, hi, dflt);
  return FMR_ERR_BAD_ARG;
}
static int check_field(const char *fn, const char *name, double &x, double lo, double hi, double dflt) {
  if (x == 0.0) x = dflt;
  if (x >= lo && x <= hi) return FMR_OK;
  set_err("%s: %s %g is outside %g .. %g (0 = %g)", fn, name, x, lo, hi, dflt);
  return FMR_ERR_BAD_ARG;
}

// A stage on the capture (noun: "the blanker", "the IQ corrector") wants a chain that takes complex float samples into an
// IF resampler
static int refuse_no_capture(const char *fn, const fmr_chain *c, const char *noun) {
  if (c->mpx_in) {
    set_err("%s: %s works on an IQ capture; an MPX decoder (fmr_create_mpx_decoder) is fed composite PCM", fn, noun);
    return FMR_ERR_UNSUPPORTED;
  }
  if (c->in_fmt != 0) {
    set_err("%s: %s reads complex float samples (FMR_IQ_CF32); this chain takes a raw input format", fn, noun);
    return FMR_ERR_UNSUPPORTED;
  }
  if (!c->has_rs) {
    set_err("%s: %s sits in front of the IF resampler; this chain has none (enable_resampler = 0)", fn, noun);
    return FMR_ERR_UNSUPPORTED;
  }
  return FMR_OK;
}

// The front of every fmr_*_derive: the pointers it needs (have: all there; names: as the message lists them) and n >= 1 ...
static int derive_args(const char *fn, bool have, const char *names, int n) {
  if (have && n >= 1) return FMR_OK;
  set_err("%s: %s is null, or n < 1", fn, names);
  return FMR_ERR_BAD_ARG;
}
// ... and, for records that count intervals, that each is one a read (`reader`) has filled
template <class Rec>
static int derive_intervals(const char *fn, const char *reader, const Rec *recs, int n) {
  for (int i = 0; i < n; i++)
    if (recs[i].n_intervals == 0) {
      set_err("%s: record %d has n_intervals 0 (not a record of %s)", fn, i, reader);
      return FMR_ERR_BAD_ARG;
    }
  return FMR_OK;
}
// 10 log10 of a power, -inf for none
static double db10(double v) { return v > 0.0 ? 10.0 * std::log10(v) : -INFINITY; }

// The PSDs of n records (psd: n x kMonPsd as read, or null: zeros) pooled, each weighted by its record's segments
template <class Rec>
static std::vector<double> mon_pool_psd(const Rec *recs, const double *psd, int n) {
  std::vector<double> p(kMonPsd, 0.0);
  unsigned long long seg = 0;
  for (int i = 0; i < n; i++) {
    seg += recs[i].segments;
    if (psd && recs[i].segments > 0)
      for (int k = 0; k < kMonPsd; k++) p[k] += (double)recs[i].segments * psd[(size_t)i * kMonPsd + k];
  }
  if (seg > 0) for (double &v : p) v /= (double)seg;
  return p;
}
// ... and the bins of lo <= f <= hi of it: their mean density (avg), or the power in them
static double mon_band(const std::vector<double> &p, double lo, double hi, bool avg) {
  const double df = kFmRate / kMonN;
  double b = 0.0; int cnt = 0;
  for (int k = 0; k < kMonPsd; k++) if (k * df >= lo && k * df <= hi) { b += p[k]; cnt++; }
  return avg ? (cnt ? b / cnt : 0.0) : b * df;
}

// ============================================================================
// C-ABI
// ============================================================================
extern "C" {

const char *fmr_last_error(void) { return g_err.c_str(); }
const char *fmr_version(void) { return "fmradion_amd 0.4.1 (gfx950)"; }

// the caller's cfg_size bytes of an fmr_config, the fields its header does not have zero ("as before")
static int widen_config(const char *fn, const fmr_config *cfg, size_t cfg_size, fmr_config *full) {
  if (cfg_size > sizeof(fmr_config)) {
    set_err("%s: the caller's fmr_config has %zu bytes, this library's %zu: the caller is newer than the library", fn, cfg_size, sizeof(fmr_config));
    return FMR_ERR_BAD_ARG;
  }
  memset(full, 0, sizeof *full);
  memcpy(full, cfg, cfg_size);
  if (cfg_size >= offsetof(fmr_config, struct_size) + sizeof(unsigned)) full->struct_size = 0;     // (stated through the argument)
  return FMR_OK;
}

static int create_chain(const fmr_config *cfg, fmr_chain **out, bool channelizer, bool rds = false,
                        const fmr_mpx_input_config *mpx_in = nullptr) {
  if (!cfg || !out) return FMR_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->struct_size != 0 && cfg->struct_size != sizeof(fmr_config)) {
    set_err("fmr_config.struct_size %u is not this library's %zu: caller and library were built against different headers "
            "(or the struct was not zero-initialised)", cfg->struct_size, sizeof(fmr_config));
    return FMR_ERR_BAD_ARG;
  }
  fmr_chain *c = new fmr_chain();
  int rc = c->init(cfg, channelizer, mpx_in);
  if (rc == FMR_OK && rds) rc = build_stage(c->rds, c->S, c->max_if);
  if (rc != FMR_OK) { delete c; return rc; }
  if (c->sync_all() != FMR_OK) { delete c; return FMR_ERR_HIP; }
  *out = c;
  return FMR_OK;
}

int fmr_create_sized(const fmr_config *cfg, size_t cfg_size, fmr_chain **out) {
  if (!cfg || !out) return FMR_ERR_BAD_ARG;
  *out = nullptr;
  fmr_config full;
  if (int rc = widen_config("fmr_create_sized", cfg, cfg_size, &full)) return rc;
  return fmr_create(&full, out);
}

int fmr_create(const fmr_config *cfg, fmr_chain **out) { return create_chain(cfg, out, false); }

int fmr_create_channelizer(const fmr_config *cfg, size_t cfg_size, fmr_chain **out) {
  if (!cfg || !out) return FMR_ERR_BAD_ARG;
  *out = nullptr;
  fmr_config full;
  if (int rc = widen_config("fmr_create_channelizer", cfg, cfg_size ? cfg_size : sizeof(fmr_config), &full)) return rc;
  return create_chain(&full, out, true);
}

void fmr_destroy(fmr_chain *c) { delete c; }

long long fmr_resampler_info(const fmr_chain *c, int which) {
  if (!c || !c->has_rs) return -1;
  switch (which) {
  case 0: return c->rs.D;
  case 1: return c->rs.NA;
  case 2: return c->rs.LB;
  case 3: return c->rs.MB;
  case 4: return c->rs.TB;
  case 5: return c->rs.LT;
  case 6: return c->fe_forms_a;
  case 7: return c->fe_forms_b;
  case 8: return c->cb_forms;
  }
  return -1;
}

static long long design_taps_out(const ResamplerDesign &d, int stage, double *taps, long long cap, long long *info);
long long fmr_design_taps_class(double in_rate, double out_rate, int resampler_class, int stage, double *taps,
                                long long cap, long long *info) {
  ResamplerDesign d;
  const bool r8b = resampler_class == FMR_RESAMPLER_R8B;
  if (resampler_class != FMR_RESAMPLER_FAST && !r8b) { set_err("unknown resampler_class %d", resampler_class); return FMR_ERR_BAD_ARG; }
  if (!(r8b ? d.design(in_rate, out_rate, kR8bAtten, kR8bPassFrac, true) : d.design(in_rate, out_rate, kIfAtten))) {
    set_err("resampling ratio outside the design range");
    return FMR_ERR_UNSUPPORTED;
  }
  return design_taps_out(d, stage, taps, cap, info);
}
long long fmr_design_taps(double in_rate, double out_rate, double atten_db, int stage, double *taps, long long cap,
                          long long *info) {
  ResamplerDesign d;
  if (!d.design(in_rate, out_rate, atten_db)) { set_err("resampling ratio outside the design range"); return FMR_ERR_UNSUPPORTED; }
  return design_taps_out(d, stage, taps, cap, info);
}
static long long design_taps_out(const ResamplerDesign &d, int stage, double *taps, long long cap, long long *info) {
  if (info) { info[0] = d.D; info[1] = d.NA; info[2] = d.LB; info[3] = d.MB; info[4] = d.TB; info[5] = d.LT; }
  const std::vector<double> &h = stage ? d.hB : d.hA;
  if (!taps) return (long long)h.size();
  if ((long long)h.size() > cap) return FMR_ERR_CAPACITY;
  for (size_t i = 0; i < h.size(); i++) taps[i] = h[i];
  return (long long)h.size();
}

void *fmr_host_alloc(size_t bytes) {
  void *p = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_err("no HIP device"); return nullptr; }
  const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
  if (e != hipSuccess) { set_err("hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
  return p;
}

void fmr_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int fmr_synchronize(fmr_chain *c) {
  if (!c) return FMR_ERR_BAD_ARG;
  if (int rc = c->sync_all()) return rc;
  return c->check_agc_sync();
}

// an MPX-input chain takes PCM through fmr_process_mpx_blocks* only
static int refuse_mpx_chain(const char *fn, const fmr_chain *c) {
  if (!c->mpx_in) return FMR_OK;
  set_err("%s: the chain is an MPX decoder (fmr_create_mpx_decoder): it takes PCM frames through fmr_process_mpx_blocks / fmr_process_mpx_blocks_device", fn);
  return FMR_ERR_BAD_ARG;
}

// how many IF samples per stream every block would produce (if_len[b]) and in all, from a copy of the resampler counter
// (nothing is advanced)
static size_t predict_if(const fmr_chain *c, const uint32_t *block_len, int nb, uint32_t *if_len) {
  ResamplerCounter r = c->rsc;
  size_t total = 0;
  for (int b = 0; b < nb; b++) {
    const size_t n = c->has_rs ? (size_t)r.advance(c->rs, block_len[b]) : (size_t)block_len[b];
    if (if_len) if_len[b] = (uint32_t)n;
    total += n;
  }
  return total;
}

// how many doubles per stream the blocks would produce, from copies of the count-law counters (nothing is advanced)
static size_t predict_audio(const fmr_chain *c, const uint32_t *block_len, int nb) {
  ResamplerCounter r = c->rsc, ar = c->arsc;
  size_t total = 0;
  unsigned long long mi_f = c->mpxi.frames;
  for (int b = 0; b < nb; b++) {
    long long n_if;
    if (c->mpx_in) {
      n_if = (long long)(c->mpxi.samples_after(mi_f + block_len[b]) - c->mpxi.samples_after(mi_f));
      mi_f += block_len[b];
    } else
      n_if = c->has_rs ? r.advance(c->rs, block_len[b]) : (long long)block_len[b];
    if (!c->has_dec || n_if == 0) continue;
    if (c->mode == FMR_MODE_FM) total += (size_t)ar.advance(c->ars, n_if) * (c->stereo ? 2 : 1);
    else total += (size_t)n_if;
  }
  return total;
}

int fmr_process_blocks_device(fmr_chain *c, const float *d_iq, size_t stream_stride, const uint32_t *block_len,
                              int n_blocks, double *d_audio, size_t audio_stride, uint32_t *audio_len, int sync) {
  if (!c || !d_iq || !block_len || n_blocks < 1) return FMR_ERR_BAD_ARG;
  if (int rc = refuse_mpx_chain("fmr_process_blocks_device", c)) return rc;
  try {
    if (c->has_dec) {
      if (!d_audio) { set_err("d_audio is null"); return FMR_ERR_BAD_ARG; }
      if (n_blocks <= c->max_blocks && predict_audio(c, block_len, n_blocks) > audio_stride) {
        set_err("audio_stride too small for the audio these blocks produce (nothing was processed)");
        return FMR_ERR_CAPACITY;
      }
    }
    const int rc = c->run_cold_aware((const float2 *)d_iq, stream_stride, block_len, n_blocks, d_audio, audio_stride, audio_len);
    if (rc) return rc;
    if (sync) { if (int rcs = c->sync_all()) return rcs; return c->check_agc_sync(); }
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_process_blocks(fmr_chain *c, const float *iq, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                       double *audio, size_t audio_stride, uint32_t *audio_len) {
  if (!c || !iq || !block_len || n_blocks < 1) return FMR_ERR_BAD_ARG;
  if (int rc = refuse_mpx_chain("fmr_process_blocks", c)) return rc;
  try {
  size_t N_in = 0;
  for (int b = 0; b < n_blocks; b++) N_in += block_len[b];
  if (N_in > c->max_in) { set_err("input longer than max_block_len*max_blocks"); return FMR_ERR_CAPACITY; }
  if (n_blocks <= c->max_blocks && c->has_dec && audio) {
    // capacity is checked BEFORE any decoder state advances: a refused call can be retried with a larger buffer
    const size_t need = predict_audio(c, block_len, n_blocks);
    if (need > audio_stride) { set_err("audio capacity %zu too small: these blocks produce %zu doubles (nothing was processed)", audio_stride, need); return FMR_ERR_CAPACITY; }
  }
  HIPCHK(hipSetDevice(c->cfg.device));
  if (N_in)
    HIPCHK(hipMemcpy2DAsync(c->d_in.p, (size_t)c->in_bps * c->max_in, iq, (size_t)c->in_bps * stream_stride,
                            (size_t)c->in_bps * N_in, (size_t)c->in_rows(), hipMemcpyHostToDevice, c->stream));
  const size_t dstride = c->stereo ? 2 * c->max_au : c->max_au;
  std::vector<uint32_t> alen(n_blocks, 0);
  const int rc = c->run_cold_aware(c->d_in.p, c->max_in, block_len, n_blocks, c->d_audio.p, dstride, alen.data());
  if (rc) return rc;
  size_t total = 0;
  for (int b = 0; b < n_blocks; b++) { total += alen[b]; if (audio_len) audio_len[b] = alen[b]; }
  if (total > audio_stride && c->S > 1) { set_err("audio_stride too small"); return FMR_ERR_CAPACITY; }
  if (int rcf = c->flush_tail(nullptr)) return rcf;      // (pipelined chain: this call's tail stage, now)
  if (total && audio) {
    if (total > audio_stride) { set_err("audio capacity too small"); return FMR_ERR_CAPACITY; }
    HIPCHK(hipMemcpy2DAsync(audio, sizeof(double) * audio_stride, c->d_audio.p, sizeof(double) * dstride,
                            sizeof(double) * total, c->S, hipMemcpyDeviceToHost, c->pipelined ? c->tail : c->stream));
  }
  if (int rcs = c->sync_all()) return rcs;
  return c->check_agc_sync();
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_fourth_convert(fmr_chain *c, const float *iq, size_t n, float *out_iq, int up, unsigned *index) {
  if (!c || !index || (n && (!iq || !out_iq))) return FMR_ERR_BAD_ARG;
  if (int rc = refuse_mpx_chain("fmr_fourth_convert", c)) return rc;
  if (n == 0) return FMR_OK;
  if (n > c->max_in || c->in_fmt != 0) { set_err("fmr_fourth_convert: block longer than the chain's capacity, or raw-format chain"); return FMR_ERR_CAPACITY; }
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipMemcpyAsync(c->d_in.p, iq, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_fourth_shift, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, c->stream, c->d_in.p,
                     c->d_in.p, (long long)n, *index & 3u, up);
  HIPCHK(hipMemcpyAsync(out_iq, c->d_in.p, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *index = up ? (unsigned)((*index + 4u - (unsigned)(n & 3)) & 3u) : (unsigned)((*index + (unsigned)(n & 3)) & 3u);
  return FMR_OK;
}

int fmr_process(fmr_chain *c, const float *iq, size_t n, double *audio, size_t audio_cap, size_t *n_audio) {
  if (!c || !n_audio) return FMR_ERR_BAD_ARG;
  *n_audio = 0;
  if (int rc = refuse_mpx_chain("fmr_process", c)) return rc;
  if (c->bank && c->S > 1) {
    set_err("fmr_process: a channel bank of %d channels produces %d audio rows; use fmr_process_blocks", c->S, c->S);
    return FMR_ERR_BAD_ARG;
  }
  if (n == 0) return FMR_OK;             // FmDecode.cpp:89-92
  uint32_t bl = (uint32_t)n, al = 0;
  const int rc = fmr_process_blocks(c, iq, n, &bl, 1, audio, audio_cap, &al);
  if (rc) return rc;
  *n_audio = al;
  return FMR_OK;
}

int fmr_resample(fmr_chain *c, const float *iq, size_t n, float *out_iq, size_t out_cap, size_t *n_out) {
  if (c) if (int rc = refuse_mpx_chain("fmr_resample", c)) return rc;
  if (!c || !n_out || !c->has_rs) return FMR_ERR_BAD_ARG;
  *n_out = 0;
  if (c->has_dec) { set_err("fmr_resample needs a chain created with mode -1 (front end only)"); return FMR_ERR_BAD_ARG; }
  if (c->bank && c->S > 1) {
    set_err("fmr_resample: a channelizer of %d channels produces %d IQ rows; use fmr_resample_blocks", c->S, c->S);
    return FMR_ERR_BAD_ARG;
  }
  if (n == 0) return FMR_OK;
  if (n > c->max_in) return FMR_ERR_CAPACITY;
  HIPCHK(hipSetDevice(c->cfg.device));
  HIPCHK(hipMemcpyAsync(c->d_in.p, iq, (size_t)c->in_bps * n, hipMemcpyHostToDevice, c->stream));
  uint32_t bl = (uint32_t)n;
  const int rc = c->run(c->d_in.p, c->max_in, &bl, 1, nullptr, 0, nullptr);
  if (rc) return rc;
  if ((size_t)c->last_n_if > out_cap) { set_err("out_cap too small"); return FMR_ERR_CAPACITY; }
  if (c->last_n_if)
    HIPCHK(hipMemcpyAsync(out_iq, c->d_if.p + c->H_if, sizeof(float2) * c->last_n_if, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n_out = (size_t)c->last_n_if;
  return FMR_OK;
}

// The checks both fmr_resample_blocks forms make before anything is enqueued or any counter moves: a refused call can be
// retried.  Fills if_len[b] (the IF samples block b produces, the same in every row) and *n_if (their sum).
static int check_resample_blocks(fmr_chain *c, const void *iq, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                                 const void *out_iq, size_t out_stride, uint32_t *if_len, size_t *n_if) {
  if (!c || !iq || !block_len || n_blocks < 1 || !out_iq) return FMR_ERR_BAD_ARG;
  if (int rc = refuse_mpx_chain("fmr_resample_blocks", c)) return rc;
  if (!c->has_rs || c->has_dec) {
    set_err("fmr_resample_blocks needs a front-end-only chain with the IF resampler (mode -1, enable_resampler)");
    return FMR_ERR_BAD_ARG;
  }
  if (n_blocks > c->max_blocks) { set_err("n_blocks %d outside 1..%d", n_blocks, c->max_blocks); return FMR_ERR_CAPACITY; }
  size_t N_in = 0;
  for (int b = 0; b < n_blocks; b++) {
    if (block_len[b] > c->cfg.max_block_len) { set_err("block %d longer than max_block_len", b); return FMR_ERR_CAPACITY; }
    N_in += block_len[b];
  }
  if (!c->bank && c->S > 1 && stream_stride < N_in) {
    set_err("stream_stride %zu is shorter than the %zu input samples of a row", stream_stride, N_in);
    return FMR_ERR_BAD_ARG;
  }
  *n_if = predict_if(c, block_len, n_blocks, if_len);
  if (*n_if > out_stride) {
    set_err("out_stride %zu too small: these blocks produce %zu IQ samples per row (nothing was processed)", out_stride, *n_if);
    return FMR_ERR_CAPACITY;
  }
  return FMR_OK;
}

int fmr_resample_blocks(fmr_chain *c, const float *iq, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                        float *out_iq, size_t out_stride, uint32_t *out_len) {
  try {
    std::vector<uint32_t> lens((size_t)std::max(n_blocks, 0));
    size_t n_if = 0;
    if (int rc = check_resample_blocks(c, iq, stream_stride, block_len, n_blocks, out_iq, out_stride, lens.data(), &n_if)) return rc;
    size_t N_in = 0;
    for (int b = 0; b < n_blocks; b++) N_in += block_len[b];
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t row = (size_t)c->in_bps * N_in;
    if (N_in)
      HIPCHK(hipMemcpy2DAsync(c->d_in.p, (size_t)c->in_bps * c->max_in, iq, c->bank ? row : (size_t)c->in_bps * stream_stride, row,
                              (size_t)c->in_rows(), hipMemcpyHostToDevice, c->stream));
    if (int rc = c->run(c->d_in.p, c->max_in, block_len, n_blocks, nullptr, 0, nullptr)) return rc;
    if (n_if)
      HIPCHK(hipMemcpy2DAsync(out_iq, sizeof(float2) * out_stride, c->d_if.p + c->H_if, sizeof(float2) * (c->H_if + c->max_if),
                              sizeof(float2) * n_if, (size_t)c->S, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (out_len) for (int b = 0; b < n_blocks; b++) out_len[b] = lens[b];
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_resample_blocks_device(fmr_chain *c, const float *d_iq, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                               float *d_out_iq, size_t out_stride, uint32_t *out_len, int sync) {
  try {
    std::vector<uint32_t> lens((size_t)std::max(n_blocks, 0));
    size_t n_if = 0;
    if (int rc = check_resample_blocks(c, d_iq, stream_stride, block_len, n_blocks, d_out_iq, out_stride, lens.data(), &n_if)) return rc;
    c->if_out = reinterpret_cast<float2 *>(d_out_iq);
    c->if_out_stride = (long long)out_stride;
    const int rc = c->run((const float2 *)d_iq, stream_stride, block_len, n_blocks, nullptr, 0, nullptr);
    c->if_out = nullptr;
    if (rc) return rc;
    if (out_len) for (int b = 0; b < n_blocks; b++) out_len[b] = lens[b];
    if (sync) return c->sync_all();
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

static int fetch_state(fmr_chain *c) {
  HIPCHK(hipSetDevice(c->cfg.device));
  if (int rc = c->sync_all()) return rc;
  HIPCHK(hipMemcpy(c->h_state.data(), c->d_state.p, sizeof(StreamState) * c->S, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(c->h_flags.data(), c->d_flags.p, sizeof(IterFlags) * c->S, hipMemcpyDeviceToHost));
  return FMR_OK;
}

int fmr_get_status_sized(fmr_chain *c, int stream, void *st, size_t st_size) {
  fmr_status full;
  const int rc = fmr_get_status(c, stream, &full);
  if (rc == FMR_OK && st && st_size) give_sized(st, st_size, full);      // never past the caller's struct
  return st ? rc : FMR_ERR_BAD_ARG;
}

int fmr_get_status(fmr_chain *c, int stream, fmr_status *st) {
  if (!c || !st || stream < 0 || stream >= c->S) return FMR_ERR_BAD_ARG;
  const int rc = fetch_state(c);
  if (rc) return rc;
  const StreamState &s = c->h_state[stream];
  st->if_rms = s.if_rms;
  st->baseband_mean = s.baseband_mean;
  st->baseband_level = s.baseband_level;
  st->pilot_level = 2 * s.pll_level;
  st->stereo_detected = s.stereo_detected;
  st->if_agc_gain = s.agc_gain;
  st->af_agc_gain = s.af_gain;
  st->multipath_error = s.mpf_error;
  st->pll_freq_err = s.pll_freq_err;
  st->multipath_resets = s.mpf_resets;
  st->agc_sync_timeouts = s.agc_sync_timeouts;
  const IterFlags &f = c->h_flags[stream];
  st->agc_iterations = f.agc_iters;
  st->pll_iterations = f.pll_iters;
  st->agc_fallback = f.agc_fallback;
  st->pll_fallback = f.pll_fallback;
  st->pll_residual = f.pll_resid;
  for (int i = 0; i < 16; i++) { st->agc_residual_history[i] = f.agc_hist[i]; st->pll_residual_history[i] = f.pll_hist[i]; }
  for (int i = 0; i < 8; i++) st->pll_residual_components[i] = f.pll_comp[i];
  for (int i = 0; i < 16; i++) st->pll_mismatch_history[i] = f.pll_rhist[i];
  st->pll_mismatch_accepted = f.pll_r_accepted;
  st->af_agc_fallback = f.af_fallback;
  return FMR_OK;
}

int fmr_get_pps_events(fmr_chain *c, int stream, fmr_pps_event *ev, int cap) {
  if (!c || stream < 0 || stream >= c->S || cap < 0 || (cap > 0 && !ev)) return FMR_ERR_BAD_ARG;
  const int rc = fetch_state(c);
  if (rc) return rc;
  const StreamState &s = c->h_state[stream];
  for (int i = 0; i < s.n_pps && i < cap; i++) {
    ev[i].pps_index = s.pps[i].pps_index;
    ev[i].sample_index = s.pps[i].sample_index;
    ev[i].block_position = s.pps[i].block_position;
    ev[i].block = s.pps[i].block + (uint32_t)c->pps_block_base;
    ev[i].stream = (uint32_t)stream;
  }
  return s.n_pps;
}

int fmr_get_multipath_coefficients(fmr_chain *c, int stream, float *coeff, int cap) {
  if (!c || stream < 0 || stream >= c->S || c->mpf_N == 0) return FMR_ERR_BAD_ARG;
  if (cap < 2 * c->mpf_N) return FMR_ERR_CAPACITY;
  HIPCHK(hipSetDevice(c->cfg.device));
  if (int rc = c->sync_all()) return rc;
  HIPCHK(hipMemcpy(coeff, c->d_mpf_coeff.p + (size_t)stream * c->mpf_N, sizeof(float2) * c->mpf_N, hipMemcpyDeviceToHost));
  return c->mpf_N;
}

long long fmr_debug_live_resources(void) { return g_live.load(); }

static int debug_chain_shape(const char *fn, const fmr_config *cfg, size_t cfg_size, int channelizer, const fmr_mpx_input_config *mpx_in,
                             fmr_chain_shape_info *out, size_t out_size) {
  if (!cfg || !out) { set_err("%s: cfg or out is NULL", fn); return FMR_ERR_BAD_ARG; }
  if ((out_size ? out_size : sizeof *out) > sizeof *out) {
    set_err("%s: out_size %zu is larger than this library's fmr_chain_shape_info (%zu): the caller is newer than the library",
            fn, out_size, sizeof *out);
    return FMR_ERR_BAD_ARG;
  }
  fmr_config full;
  if (int rc = widen_config(fn, cfg, cfg_size ? cfg_size : sizeof(fmr_config), &full)) return rc;
  try {
    EnvKnobs env;
    env.load();
    ChainShape sh;
    if (int rc = plan_create(sh, &full, env, channelizer != 0, mpx_in)) return rc;
    fmr_chain_shape_info o{};
    o.struct_size = (unsigned)sizeof o;
    if (sh.has_rs) {
      o.D = sh.rs.D; o.NA = sh.rs.NA; o.LB = sh.rs.LB; o.MB = sh.rs.MB; o.TB = sh.rs.TB; o.LT = sh.rs.LT;
      o.stage_b = kFeBitB[(int)sh.fe.b];
    }
    o.fused = (int)sh.fe.fused; o.decim16 = sh.fe.decim16; o.poly5h_disc = sh.fe.poly5h_disc;
    o.fir = sh.fe.fir == ChainShape::IfForm::poly4_disc ? 1 : sh.fe.fir == ChainShape::IfForm::poly4_finish ? 2 : 0;
    o.qa = sh.qa; o.pipelined = sh.pipelined;
    o.max_if = sh.max_if; o.max_au = sh.max_au;
    if (sh.mpx_in) { o.mpx_in = 1; o.mpx_format = sh.mi_format; o.mpx_L = sh.mi_L; o.mpx_M = sh.mi_M; o.mpx_T = sh.mi_T; o.mpx_K = sh.mi_K; }
    give_sized(out, out_size, o);
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_debug_chain_shape(const fmr_config *cfg, size_t cfg_size, int channelizer, fmr_chain_shape_info *out, size_t out_size) {
  return debug_chain_shape("fmr_debug_chain_shape", cfg, cfg_size, channelizer, nullptr, out, out_size);
}

long long fmr_debug_read(fmr_chain *c, int stream, int which, void *out, size_t cap_bytes) {
  if (!c || stream < 0 || stream >= c->S) return FMR_ERR_BAD_ARG;
  HIPCHK(hipSetDevice(c->cfg.device));
  if (int rc = c->sync_all()) return rc;
  long long n = c->last_n_if;
  const void *src = nullptr;
  size_t esz = 0;
  if (which == 6 || which == 7) {     // the input row an acting capture stage wrote in the most recent call (`stream` is an input row):
    // 6 the blanker's, which the front end read; 7 the IQ corrector's
    const CaptureStage &st = which == 6 ? (const CaptureStage &)c->nb : c->iqc;
    if (!st.on || !st.act || stream >= st.rows) {
      set_err(which == 6 ? "fmr_debug_read: tap 6 (blanked input rows) needs a chain with fmr_enable_blanker in FMR_NB_ACT, and an input row"
                         : "fmr_debug_read: tap 7 (corrected input rows) needs a chain with fmr_enable_iq_correction in FMR_IQC_ACT, and an input row");
      return FMR_ERR_BAD_ARG;
    }
    n = st.last_n;
    if ((size_t)n * sizeof(float2) > cap_bytes) return FMR_ERR_CAPACITY;
    if (n) HIPCHK(hipMemcpy(out, st.last_rows + (long long)stream * st.last_stride, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost));
    return n;
  }
  if (which == 5 && !c->d_fe_stamps.p) {      // the symbol reliabilities of the most recent call (chains with RDS)
    if (!c->rds.on) { set_err("fmr_debug_read: tap 5 (RDS symbol reliabilities) needs a chain made by fmr_create_rds"); return FMR_ERR_BAD_ARG; }
    c->rds.drain();
    if (!c->rds.tap_seq) return 0;
    const char *sl = c->rds.h_slots.p + ((size_t)(c->rds.tap_seq % RdsStage::kSlots) * c->S + stream) * c->rds.slot_stride;
    RdsSlotHdr h;
    memcpy(&h, sl, sizeof h);
    const RdsRec *rec = reinterpret_cast<const RdsRec *>(sl + sizeof(RdsSlotHdr));
    const float *rho = reinterpret_cast<const float *>(sl + rds_slot_rho_off(c->rds.maxw));
    n = 0;
    for (int w = 0; w < h.nw && w < c->rds.maxw; w++) n += std::min(std::max(rec[w].count, 0), kRdsMaxSym);
    if ((size_t)n * sizeof(float) > cap_bytes) return FMR_ERR_CAPACITY;
    float *o = reinterpret_cast<float *>(out);
    for (int w = 0; w < h.nw && w < c->rds.maxw; w++)
      for (int t = 0; t < rec[w].count && t < kRdsMaxSym; t++) *o++ = rho[(size_t)w * (kRdsMaxSym + 1) + t + 1];
    return n;
  }
  if (which == 5) {       // FMR_FE_STAMPS=1 (diagnostics; the tap then keeps this meaning on every chain): {start, end [10 ns units of the constant clock], hardware id} per workgroup of the last fused launch
    if (!c->d_fe_stamps.p || stream != 0) return FMR_ERR_BAD_ARG;
    constexpr long long R = 2 * 16 * fmr_chain::kStampCalls;
    n = 3ll * c->fe_stamps_n;        // ... followed by the two rings of stream stamps (32 calls x 16 ids: constant clock, shader cycles) and the sequence number of the last call
    if ((size_t)(n + R + 1) * 8 > cap_bytes) return FMR_ERR_CAPACITY;
    if (n) HIPCHK(hipMemcpy(out, c->d_fe_stamps.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy((char *)out + (size_t)n * 8, c->d_fe_stamps.p + 3 * (size_t)c->kMaxFusedWg * c->S, R * 8, hipMemcpyDeviceToHost));
    reinterpret_cast<unsigned long long *>(out)[n + R] = c->call_seq;
    return n + R + 1;
  }
  switch (which) {
  case 0: src = (c->last_if && c->if_valid) ? c->last_if + (size_t)stream * (c->H_if + c->max_if) + c->H_if : nullptr; esz = sizeof(float2); break;
  case 1: src = (c->d_dec.p && c->dec_valid) ? c->d_dec.p + (size_t)stream * c->max_if : nullptr; esz = sizeof(float); break;
  case 2: src = c->d_raw_de.p ? c->d_raw_de.p + (size_t)stream * (c->H_a + c->max_if) + c->H_a : nullptr; esz = sizeof(double); break;
  case 3: src = c->d_base_de.p ? c->d_base_de.p + (size_t)stream * (c->H_a + c->max_if) + c->H_a : nullptr; esz = sizeof(double); break;
  case 4: src = (c->d_gain.p && c->gain_valid) ? c->d_gain.p + (size_t)stream * c->max_if : nullptr; esz = sizeof(float); break;
  default: return FMR_ERR_BAD_ARG;
  }
  if (!src) return FMR_ERR_BAD_ARG;
  if ((size_t)n * esz > cap_bytes) return FMR_ERR_CAPACITY;
  if (n) HIPCHK(hipMemcpy(out, src, (size_t)n * esz, hipMemcpyDeviceToHost));
  return n;
}

// plain streaming read: what the box delivers to a kernel that only reads (bench.py: context for the roofline fraction)
__global__ __launch_bounds__(256) void k_probe_read(const float *__restrict__ p0, size_t n16, float *sink) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  const v4f *p = reinterpret_cast<const v4f *>(p0);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n16; i += 4 * stride) {
    const v4f a = __builtin_nontemporal_load(p + i), b = __builtin_nontemporal_load(p + i + stride),
              c = __builtin_nontemporal_load(p + i + 2 * stride), d = __builtin_nontemporal_load(p + i + 3 * stride);
    acc += (a + b) + (c + d);
  }
  for (; i < n16; i += stride) acc += __builtin_nontemporal_load(p + i);
  if (acc.x + acc.y + acc.z + acc.w == 1.2345678e-30f) *sink = acc.x;       // keeps the loads alive; never true in practice
}

namespace {
// the probes run on `device` and leave the caller's current device as it was
struct DeviceScope {
  int prev = -1;
  int enter(int device) { HIPCHK(hipGetDevice(&prev)); HIPCHK(hipSetDevice(device)); return FMR_OK; }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
}  // namespace

int fmr_probe_read_bandwidth(int device, const void *d_buf, size_t bytes, int reps, double *gbytes_per_s) {
  if (!d_buf || !gbytes_per_s || bytes < (1u << 20) || reps < 1) return FMR_ERR_BAD_ARG;
  // everything this function takes is given back on every path out of it, the caller's current device included
  DeviceScope dev;
  DevBuf<float> sink;
  Stream st;      // (the null stream would wait for every blocking stream)
  Event ev_a, ev_b;
  if (int rc = dev.enter(device)) return rc;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  const int n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (int rc = sink.alloc(1)) return rc;
  if (int rc = st.create()) return rc;
  if (int rc = ev_a.create()) return rc;
  if (int rc = ev_b.create()) return rc;
  double best = 0.0;
  for (int r = 0; r < reps + 1; r++) {          // (the first pass warms up and is not counted)
    HIPCHK(hipEventRecord(ev_a, st));
    hipLaunchKernelGGL(k_probe_read, dim3(n_cu * 8), dim3(256), 0, st, (const float *)d_buf, bytes / 16, sink.p);
    HIPCHK(hipEventRecord(ev_b, st));
    HIPCHK(hipEventSynchronize(ev_b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev_a, ev_b));
    if (r > 0 && ms > 0.f) best = std::max(best, (double)(bytes / 16 * 16) / (ms * 1e-3) / 1e9);
  }
  *gbytes_per_s = best;
  return FMR_OK;
}

int fmr_probe_shader_clock(int device, double *mhz) {
  if (!mhz) return FMR_ERR_BAD_ARG;
  DeviceScope dev;
  HostBuf<unsigned long long> out;
  Stream st;
  if (int rc = dev.enter(device)) return rc;
  if (int rc = out.alloc(2, hipHostMallocDefault)) return rc;
  if (int rc = st.create()) return rc;
  hipLaunchKernelGGL(k_probe_clock, dim3(1), dim3(64), 0, st, out.p, 2000);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  *mhz = out.p[1] ? (double)out.p[0] / ((double)out.p[1] * 0.01) : 0.0;     // cycles per microsecond
  return FMR_OK;
}

void fmr_enable_kernel_timing(fmr_chain *c, int enable) { if (c) c->timing = enable; }

int fmr_get_kernel_trace(fmr_chain *c, const char **names, int *streams, float *start_ms, float *end_ms, int cap) {
  if (!c) return FMR_ERR_BAD_ARG;
  if (int rc = c->sync_all()) return rc;
  int n = 0;
  for (size_t i = 0; i < c->trace.size(); i++) {
    float t0 = 0.f, t1 = 0.f;
    (void)hipEventElapsedTime(&t0, c->trace_base, c->trace[i].a);
    (void)hipEventElapsedTime(&t1, c->trace_base, c->trace[i].b);
    if (n < cap) { names[n] = c->trace[i].name; streams[n] = c->trace_stream[i]; start_ms[n] = t0; end_ms[n] = t1; }
    n++;
  }
  c->trace.clear(); c->trace_stream.clear();
  c->trace_base.reset();
  return n;
}

int fmr_get_kernel_times(fmr_chain *c, const char **names, float *ms, int cap) {
  if (!c) return FMR_ERR_BAD_ARG;
  if (int rc = c->sync_all()) return rc;
  int n = 0;
  const bool dom = c->timing == 2 || c->timing == 4 || c->timing == 5;   // dominant kernel only: one entry per call since the last query
  for (auto &k : dom ? c->dom_times : c->ktimes) {
    float t = 0.f;
    (void)hipEventElapsedTime(&t, k.a, k.b);
    if (n < cap) { names[n] = k.name; ms[n] = t; }
    n++;
  }
  if (dom) c->dom_times.clear();      // (the last call's times stay until the next call replaces them)
  return n;
}

int fmr_create_rds(const fmr_config *cfg, size_t cfg_size, fmr_chain **out) {
  if (!cfg || !out) return FMR_ERR_BAD_ARG;
  *out = nullptr;
  fmr_config full;
  if (int rc = widen_config("fmr_create_rds", cfg, cfg_size ? cfg_size : sizeof(fmr_config), &full)) return rc;
  // the rules of the option, before the device is opened
  if (full.mode != FMR_MODE_FM) {
    set_err("enable_rds: the RDS decoder reads the MPX of an FM chain (mode FMR_MODE_FM); mode %d %s", full.mode,
            full.mode == FMR_MODE_NONE ? "is a front-end-only chain (channelizer / IfResampler): it has no MPX" : "has no RDS");
    return FMR_ERR_UNSUPPORTED;
  }
  return create_chain(&full, out, false, true);
}

int fmr_get_rds_groups(fmr_chain *c, int stream, fmr_rds_group *groups, int cap) {
  if (!c || stream < 0 || stream >= c->S || cap < 0 || (cap > 0 && !groups)) return FMR_ERR_BAD_ARG;
  if (!c->rds.on) { set_err("fmr_get_rds_groups: the chain was created without the RDS decoder (fmr_create_rds)"); return FMR_ERR_BAD_ARG; }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    c->rds.drain();
    fmr_rds::Decoder &d = c->rds.dec[stream];
    if (cap == 0) return (int)d.queued();
    return (int)d.pop(groups, (size_t)cap);
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_get_rds_status(fmr_chain *c, int stream, fmr_rds_status *st, size_t st_size) {
  if (!c || !st || stream < 0 || stream >= c->S) return FMR_ERR_BAD_ARG;
  if (!c->rds.on) { set_err("fmr_get_rds_status: the chain was created without the RDS decoder (fmr_create_rds)"); return FMR_ERR_BAD_ARG; }
  HIPCHK(hipSetDevice(c->cfg.device));
  if (int rc = c->sync_all()) return rc;
  c->rds.drain();
  const fmr_rds::Decoder &d = c->rds.dec[stream];
  const RdsSlotHdr &h = c->rds.hdr[stream];
  fmr_rds_status full{};
  full.synced = d.synced();
  full.blocks_ok = d.blocks_ok();
  full.blocks_bad = d.blocks_bad();
  full.blocks_corrected = d.blocks_corrected();
  full.groups_decoded = d.groups_decoded();
  full.groups_dropped = d.groups_dropped();
  full.injection = h.level > 0.f ? std::sqrt((double)h.level) / c->rds.gain : 0.0;
  full.timing = h.timing_frac;
  full.carrier_phase = h.theta;
  full.carrier_offset_hz = h.freq_hz;
  if (st_size) give_sized(st, st_size, full);
  return FMR_OK;
}

int fmr_set_rds_correction(fmr_chain *c, const fmr_rds_fec *fec, size_t fec_size) {
  if (!fec) { set_err("fmr_set_rds_correction: fec is null"); return FMR_ERR_BAD_ARG; }
  fmr_rds_fec full;
  if (int rc = take_sized("fmr_set_rds_correction", "fmr_rds_fec", fec, fec_size, full)) return rc;
  fmr_rds::Correction k;
  k.mode = full.mode;
  if (full.max_burst) k.max_burst = full.max_burst;
  if (full.soft_symbols) k.soft_symbols = full.soft_symbols;
  if (full.soft_max_cost != 0.0) k.soft_max_cost = full.soft_max_cost;
  if (k.mode != FMR_RDS_FEC_OFF && k.mode != FMR_RDS_FEC_BURST && k.mode != FMR_RDS_FEC_SOFT) {
    set_err("fmr_set_rds_correction: mode %d is none of FMR_RDS_FEC_OFF / BURST / SOFT", k.mode);
    return FMR_ERR_BAD_ARG;
  }
  if (k.max_burst < 1 || k.max_burst > fmr_rds::kMaxBurst) {
    set_err("fmr_set_rds_correction: max_burst %d is outside 1 .. %d (0 = default)", k.max_burst, fmr_rds::kMaxBurst);
    return FMR_ERR_BAD_ARG;
  }
  if (k.soft_symbols < 1 || k.soft_symbols > fmr_rds::kMaxSoftSymbols) {
    set_err("fmr_set_rds_correction: soft_symbols %d is outside 1 .. %d (0 = default)", k.soft_symbols, fmr_rds::kMaxSoftSymbols);
    return FMR_ERR_BAD_ARG;
  }
  if (!(k.soft_max_cost >= 0.0) || !std::isfinite(k.soft_max_cost)) {
    set_err("fmr_set_rds_correction: soft_max_cost %g is not a finite value >= 0", k.soft_max_cost);
    return FMR_ERR_BAD_ARG;
  }
  if (!c) { set_err("fmr_set_rds_correction: chain is null"); return FMR_ERR_BAD_ARG; }
  if (!c->rds.on) { set_err("fmr_set_rds_correction: the chain was created without the RDS decoder (fmr_create_rds)"); return FMR_ERR_BAD_ARG; }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    c->rds.drain();
    for (fmr_rds::Decoder &d : c->rds.dec) d.set_correction(k);
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

// ---- modulation monitor: C-ABI ----
int fmr_enable_monitor(fmr_chain *c, const fmr_monitor_config *cfg, size_t cfg_size) {
  if (!cfg) { set_err("fmr_enable_monitor: cfg is null"); return FMR_ERR_BAD_ARG; }
  fmr_monitor_config m;
  if (int rc = take_sized("fmr_enable_monitor", "fmr_monitor_config", cfg, cfg_size, m)) return rc;
  if (m.interval_samples == 0) m.interval_samples = 384000;
  if (m.hist_range == 0.0) m.hist_range = 2.0;
  if (m.interval_samples % kMonH != 0 || m.interval_samples < (uint32_t)kMonH || m.interval_samples > (1u << 30)) {
    set_err("fmr_enable_monitor: interval_samples %u is not a multiple of 512 in 512 .. 2^30 (0 = 384000)", m.interval_samples);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field("fmr_enable_monitor", "hist_bins", m.hist_bins, 2, kMonMaxHist, 256)) return rc;
  if (!(m.hist_range > 0.0) || !std::isfinite(m.hist_range)) {
    set_err("fmr_enable_monitor: hist_range %g is not a finite value > 0 (0 = 2.0)", m.hist_range);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field("fmr_enable_monitor", "max_records", m.max_records, 1, 4096, 64)) return rc;
  if (!c) { set_err("fmr_enable_monitor: chain is null"); return FMR_ERR_BAD_ARG; }
  if (c->mode != FMR_MODE_FM) {
    set_err("fmr_enable_monitor: the monitor reads the MPX of an FM chain (mode FMR_MODE_FM); mode %d %s", c->mode,
            c->mode == FMR_MODE_NONE ? "is a front-end-only chain (channelizer / IfResampler): it has no MPX" : "has no MPX");
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage("fmr_enable_monitor", c, c->mon, "monitor", "MPX sample", c->S, c->max_if, m.interval_samples, m.hist_bins,
                      m.hist_range, m.max_records);
}

int fmr_monitor_read(fmr_chain *c, int stream, fmr_monitor_record *recs, uint32_t *hist, double *psd, int cap,
                     fmr_monitor_info *info, size_t info_size) {
  return read_records("fmr_monitor_read", c, &fmr_chain::mon, "monitor", "fmr_enable_monitor", stream, recs, cap, info, info_size,
                      copy_seg_monitor(recs, hist, psd), nullptr, [](fmr_monitor_info &full, const SegMonitor &m) {
    full.hist_bins = m.bins;
    full.psd_bins = kMonPsd;
    full.interval_samples = m.interval;
    full.max_records = (int)m.cur.L;
    full.hist_range = m.hist_range;
    full.bin_hz = kFmRate / kMonN;
  });
}

int fmr_monitor_derive(const fmr_monitor_record *recs, const double *psd, int n, fmr_monitor_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_monitor_derive", recs && out, "recs or out", n)) return rc;
  double sum = 0.0, sumsq = 0.0, mn = INFINITY, mx = -INFINITY;
  unsigned long long nf = 0, seg = 0;
  for (int i = 0; i < n; i++) {
    const fmr_monitor_record &r = recs[i];
    sum += r.sum; sumsq += r.sumsq; nf += r.n_finite; seg += r.segments;
    if (r.n_finite > 0) { mn = std::min(mn, (double)r.min); mx = std::max(mx, (double)r.max); }
  }
  const std::vector<double> p = mon_pool_psd(recs, psd, n);
  const double mean = nf ? sum / (double)nf : 0.0;
  const double var = nf ? sumsq / (double)nf - mean * mean : 0.0;
  fmr_monitor_levels full{};
  full.struct_size = (unsigned)sizeof full;
  full.tuning_offset_hz = 75000.0 * mean;
  full.peak_deviation_hz = nf ? 75000.0 * std::max(mx - mean, mean - mn) : 0.0;
  full.rms = var > 0.0 ? std::sqrt(var) : 0.0;
  full.mpx_power_dbr = var > 0.0 ? 10.0 * std::log10(2.0 * (75.0 / 19.0) * (75.0 / 19.0) * var) : -INFINITY;
  full.pilot_deviation_hz = 75000.0 * std::sqrt(2.0 * mon_band(p, 17875.0, 20125.0, false));
  full.rds_deviation_hz = 75000.0 * std::sqrt(2.0 * mon_band(p, 54600.0, 59400.0, false));
  full.hf_noise_density = mon_band(p, 100000.0, 150000.0, true);
  full.n_finite = nf;
  full.segments = seg;
  give_sized(out, out_size, full);
  return FMR_OK;
}

// ---- output stage: C-ABI ----
double fmr_squelch_level_from_db(double db) { return std::pow(10.0, -(db / 20.0)); }      // main.cpp:486

int fmr_enable_output(fmr_chain *c, const fmr_output_config *cfg, size_t cfg_size) {
  if (!cfg) { set_err("fmr_enable_output: cfg is null"); return FMR_ERR_BAD_ARG; }
  fmr_output_config m;
  if (int rc = take_sized("fmr_enable_output", "fmr_output_config", cfg, cfg_size, m)) return rc;
  if (m.format != FMR_PCM_S16 && m.format != FMR_PCM_F32) {
    set_err("fmr_enable_output: format %d is neither FMR_PCM_S16 (0) nor FMR_PCM_F32 (1)", m.format);
    return FMR_ERR_BAD_ARG;
  }
  if (!std::isfinite(m.squelch_level) || m.squelch_level < 0.0) {
    set_err("fmr_enable_output: squelch_level %g is not a finite linear level >= 0 (0 = never closed)", m.squelch_level);
    return FMR_ERR_BAD_ARG;
  }
  if (m.gain == 0.0) m.gain = 0.5;
  if (!std::isfinite(m.gain) || !(m.gain > 0.0)) {
    set_err("fmr_enable_output: gain %g is not finite and > 0 (0 = 0.5)", m.gain);
    return FMR_ERR_BAD_ARG;
  }
  if (m.max_frames == 0) m.max_frames = 1u << 18;
  if (m.max_blocks == 0) m.max_blocks = 4096;
  if (m.max_frames > (1u << 26)) {
    set_err("fmr_enable_output: max_frames %u is outside 1 .. 2^26 (0 = 2^18)", m.max_frames);
    return FMR_ERR_BAD_ARG;
  }
  if (m.max_blocks > 65536) {
    set_err("fmr_enable_output: max_blocks %u is outside 1 .. 65536 (0 = 4096)", m.max_blocks);
    return FMR_ERR_BAD_ARG;
  }
  if (!c) { set_err("fmr_enable_output: chain is null"); return FMR_ERR_BAD_ARG; }
  if (c->mpx_in && m.squelch_level != 0.0) {
    set_err("fmr_enable_output: squelch_level %g on an MPX decoder: the squelch gates on the IF level, and a chain fed composite PCM has no IF (squelch_level must be 0)", m.squelch_level);
    return FMR_ERR_UNSUPPORTED;
  }
  if (!c->has_dec) {
    set_err("fmr_enable_output: a front-end-only chain (mode -1: channelizer / IfResampler) has no audio");
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage("fmr_enable_output", c, c->out, "output stage", "block", c->S, c->stereo, c->max_blocks,
                      c->pipelined ? fmr_chain::kPipe : 1, m);
}

int fmr_output_read(fmr_chain *c, int stream, void *pcm, size_t cap_frames, fmr_output_block *blocks, int cap_blocks,
                    size_t *n_frames, fmr_output_info *info, size_t info_size) {
  if (n_frames) *n_frames = 0;
  if (!c || stream < 0 || stream >= c->S || cap_blocks < 0) { set_err("fmr_output_read: bad chain, stream or cap_blocks"); return FMR_ERR_BAD_ARG; }
  if (!c->out.on) { set_err("fmr_output_read: the chain has no output stage (fmr_enable_output)"); return FMR_ERR_BAD_ARG; }
  if (cap_frames > 0 && !pcm) { set_err("fmr_output_read: pcm is null"); return FMR_ERR_BAD_ARG; }
  if (cap_blocks > 0 && !blocks) { set_err("fmr_output_read: blocks is null"); return FMR_ERR_BAD_ARG; }
  if (info && (info_size ? info_size : sizeof(fmr_output_info)) > sizeof(fmr_output_info)) {
    set_err("fmr_output_read: info_size %zu is larger than this library's fmr_output_info (%zu): the caller is newer than the library",
            info_size, sizeof(fmr_output_info));
    return FMR_ERR_BAD_ARG;
  }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    const size_t fb = c->out.frame_bytes();
    RecCursor &fc = c->out.fcur, &bc = c->out.bcur;
    fc.catch_up(stream, c->out.produced());
    const unsigned long long first = fc.read[stream];
    int nf = 0;
    if (cap_frames > 0) {
      nf = fc.take(stream, c->out.produced(), (unsigned long long)cap_frames, [&](size_t k, size_t slot, size_t m) -> int {
        HIPCHK(hipMemcpy((char *)pcm + k * fb, c->out.d_pcm.p + ((size_t)stream * fc.L + slot) * fb, m * fb, hipMemcpyDeviceToHost));
        return FMR_OK;
      });
      if (nf < 0) return nf;
    }
    int nb = 0;
    bc.catch_up(stream, c->out.recs);
    if (cap_blocks > 0) {
      nb = bc.take(stream, c->out.recs, (unsigned long long)cap_blocks, [&](size_t k, size_t slot, size_t m) -> int {
        HIPCHK(hipMemcpy(blocks + k, c->out.d_rec.p + (size_t)stream * bc.L + slot, m * sizeof(fmr_output_block), hipMemcpyDeviceToHost));
        return FMR_OK;
      });
      if (nb < 0) return nb;
    }
    if (n_frames) *n_frames = (size_t)nf;
    if (info) {
      fmr_output_info full{};
      full.struct_size = (unsigned)sizeof full;
      full.format = c->out.cfg.format;
      full.channels = c->out.channels();
      full.first_frame = first;
      full.frames_waiting = c->out.produced() - fc.read[stream];
      full.frames_dropped = fc.dropped[stream];
      full.blocks_waiting = c->out.recs - bc.read[stream];
      full.blocks_dropped = bc.dropped[stream];
      give_sized(info, info_size, full);
    }
    return nb;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

static int check_output_rate(int rate) {
  int L, M, T;
  if (rate < kOutRateMin || rate > kOutRateIn || !design_output_rate(rate, L, M, T, nullptr)) {
    set_err("fmr_set_output_rate: rate %d is not 0, 48000 or a whole rate in 8000 .. 48000 with L = rate / gcd(rate, 48000) <= %d",
            rate, kOutRateMaxL);
    return FMR_ERR_BAD_ARG;
  }
  return FMR_OK;
}

int fmr_set_output_rate(fmr_chain *c, const fmr_output_rate_config *cfg, size_t cfg_size) {
  if (!cfg) { set_err("fmr_set_output_rate: cfg is null"); return FMR_ERR_BAD_ARG; }
  fmr_output_rate_config m;
  if (int rc = take_sized("fmr_set_output_rate", "fmr_output_rate_config", cfg, cfg_size, m)) return rc;
  if (m.rate == 0) m.rate = kOutRateIn;
  if (int rc = check_output_rate(m.rate)) return rc;
  if (m.mono != 0 && m.mono != 1) { set_err("fmr_set_output_rate: mono %d is neither 0 nor 1", m.mono); return FMR_ERR_BAD_ARG; }
  if (m.reserved != 0) { set_err("fmr_set_output_rate: reserved %d is not 0", m.reserved); return FMR_ERR_BAD_ARG; }
  if (!c) { set_err("fmr_set_output_rate: chain is null"); return FMR_ERR_BAD_ARG; }
  if (!c->out.on) { set_err("fmr_set_output_rate: the chain has no output stage (fmr_enable_output comes first)"); return FMR_ERR_BAD_ARG; }
  if (c->out.rate_set) { set_err("fmr_set_output_rate: the output rate of this chain is already set"); return FMR_ERR_BAD_ARG; }
  if (c->call_seq != 0) {
    set_err("fmr_set_output_rate: the chain has already taken samples (the ring counts from the chain's first block)");
    return FMR_ERR_BAD_ARG;
  }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    const bool mono = m.mono == 1 && c->stereo;
    if (m.rate != kOutRateIn || mono)      // (else: the stage as it is)
      if (int rc = build_stage(c->out.rate, m.rate, mono, c->S, c->stereo, c->max_au)) return rc;
    c->out.rate_set = true;
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_get_output_rate(fmr_chain *c, int stream, fmr_output_rate_info *info, size_t info_size) {
  if (!c || !info || stream < 0 || stream >= c->S) { set_err("fmr_get_output_rate: bad chain, stream or info"); return FMR_ERR_BAD_ARG; }
  if (!c->out.on) { set_err("fmr_get_output_rate: the chain has no output stage (fmr_enable_output)"); return FMR_ERR_BAD_ARG; }
  if ((info_size ? info_size : sizeof(fmr_output_rate_info)) > sizeof(fmr_output_rate_info)) {
    set_err("fmr_get_output_rate: info_size %zu is larger than this library's fmr_output_rate_info (%zu): the caller is newer than the library",
            info_size, sizeof(fmr_output_rate_info));
    return FMR_ERR_BAD_ARG;
  }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    fmr_output_rate_info full{};
    full.struct_size = (unsigned)sizeof full;
    full.rate = c->out.rate.hz; full.channels = c->out.channels();
    full.L = c->out.rate.geom.L; full.M = c->out.rate.geom.M; full.taps_per_phase = c->out.rate.geom.T;
    full.delay_frames = full.taps_per_phase > 1 ? ((double)full.taps_per_phase * full.L - 1.0) / (2.0 * full.M) : 0.0;
    full.frames_in = c->out.frames;
    if (c->out.rate.on) {
      unsigned long long tot[2];
      HIPCHK(hipMemcpy(tot, c->out.rate.d_tot.p + 2 * (size_t)stream, sizeof tot, hipMemcpyDeviceToHost));
      full.pcm_clipped = tot[0]; full.pcm_nonfinite = tot[1];
    }
    give_sized(info, info_size, full);
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_output_rate_taps(int rate, double *taps, int cap, int *L, int *M, int *T) {
  if (rate == 0) rate = kOutRateIn;
  if (int rc = check_output_rate(rate)) return rc;
  int l, m, t;
  std::vector<double> h;
  design_output_rate(rate, l, m, t, nullptr);
  if (L) *L = l;
  if (M) *M = m;
  if (T) *T = t;
  const long long n = (long long)t * l;
  if (taps && (long long)cap >= n) {
    design_output_rate(rate, l, m, t, &h);
    memcpy(taps, h.data(), (size_t)n * sizeof(double));
  }
  return (int)n;
}

// ---- MPX output: C-ABI ----
static int check_mpx_rate(const char *fn, int rate) {
  int L, M, T;
  if (!design_mpx_rate(rate, L, M, T, nullptr)) {
    set_err("%s: rate %d is not 0, 384000 or a whole rate in 96000 .. 384000 with L = rate / gcd(rate, 384000) <= %d", fn, rate,
            kOutRateMaxL);
    return FMR_ERR_BAD_ARG;
  }
  return FMR_OK;
}

int fmr_enable_mpx_output(fmr_chain *c, const fmr_mpx_output_config *cfg, size_t cfg_size) {
  const char *fn = "fmr_enable_mpx_output";
  if (!cfg) { set_err("%s: cfg is null", fn); return FMR_ERR_BAD_ARG; }
  fmr_mpx_output_config m;
  if (int rc = take_sized(fn, "fmr_mpx_output_config", cfg, cfg_size, m)) return rc;
  if (m.format != FMR_PCM_S16 && m.format != FMR_PCM_F32) {
    set_err("%s: format %d is neither FMR_PCM_S16 (0) nor FMR_PCM_F32 (1)", fn, m.format);
    return FMR_ERR_BAD_ARG;
  }
  if (m.rate == 0) m.rate = kMpxRateIn;
  if (int rc = check_mpx_rate(fn, m.rate)) return rc;
  if (m.gain == 0.0) m.gain = 0.5;
  if (!std::isfinite(m.gain) || !(m.gain > 0.0)) { set_err("%s: gain %g is not finite and > 0 (0 = 0.5)", fn, m.gain); return FMR_ERR_BAD_ARG; }
  if (m.max_frames == 0) m.max_frames = 1u << 20;
  if (m.max_frames > (1u << 26)) { set_err("%s: max_frames %u is outside 1 .. 2^26 (0 = 2^20)", fn, m.max_frames); return FMR_ERR_BAD_ARG; }
  if (!c) { set_err("%s: chain is null", fn); return FMR_ERR_BAD_ARG; }
  if (c->mode != FMR_MODE_FM) {
    set_err("%s: the MPX output reads the MPX of an FM chain (mode FMR_MODE_FM); mode %d %s", fn, c->mode,
            c->mode == FMR_MODE_NONE ? "is a front-end-only chain (channelizer / IfResampler): it has no MPX" : "has no MPX");
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage(fn, c, c->mpxo, "MPX output", "MPX sample", c->S, m);
}

int fmr_mpx_output_read(fmr_chain *c, int stream, void *pcm, size_t cap_frames, size_t *n_frames, fmr_mpx_output_info *info,
                        size_t info_size) {
  if (n_frames) *n_frames = 0;
  if (!c || stream < 0 || stream >= c->S) { set_err("fmr_mpx_output_read: bad chain or stream"); return FMR_ERR_BAD_ARG; }
  if (!c->mpxo.on) { set_err("fmr_mpx_output_read: the chain has no MPX output (fmr_enable_mpx_output)"); return FMR_ERR_BAD_ARG; }
  if (cap_frames > 0 && !pcm) { set_err("fmr_mpx_output_read: pcm is null"); return FMR_ERR_BAD_ARG; }
  if (info && (info_size ? info_size : sizeof(fmr_mpx_output_info)) > sizeof(fmr_mpx_output_info)) {
    set_err("fmr_mpx_output_read: info_size %zu is larger than this library's fmr_mpx_output_info (%zu): the caller is newer than the library",
            info_size, sizeof(fmr_mpx_output_info));
    return FMR_ERR_BAD_ARG;
  }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    MpxOutStage &st = c->mpxo;
    const size_t fb = st.frame_bytes();
    RecCursor &fc = st.cur;
    fc.catch_up(stream, st.oframes);
    const unsigned long long first = fc.read[stream];
    int nf = 0;
    if (cap_frames > 0) {
      nf = fc.take(stream, st.oframes, (unsigned long long)cap_frames, [&](size_t k, size_t slot, size_t m) -> int {
        HIPCHK(hipMemcpy((char *)pcm + k * fb, st.d_pcm.p + ((size_t)stream * fc.L + slot) * fb, m * fb, hipMemcpyDeviceToHost));
        return FMR_OK;
      });
      if (nf < 0) return nf;
    }
    if (n_frames) *n_frames = (size_t)nf;
    if (info) {
      fmr_mpx_output_info full{};
      full.struct_size = (unsigned)sizeof full;
      full.format = st.cfg.format; full.rate = st.cfg.rate;
      full.L = st.geom.L; full.M = st.geom.M; full.taps_per_phase = st.geom.T;
      full.delay_frames = st.geom.T > 1 ? ((double)st.geom.T * st.geom.L - 1.0) / (2.0 * st.geom.M) : 0.0;
      full.full_scale_hz = 75000.0 / st.cfg.gain;
      full.first_frame = first;
      full.frames_waiting = st.oframes - fc.read[stream];
      full.frames_dropped = fc.dropped[stream];
      full.samples_in = st.n;
      unsigned long long tot[2];
      HIPCHK(hipMemcpy(tot, st.d_tot.p + 2 * (size_t)stream, sizeof tot, hipMemcpyDeviceToHost));
      full.pcm_clipped = tot[0]; full.pcm_nonfinite = tot[1];
      give_sized(info, info_size, full);
    }
    return nf;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_mpx_output_taps(int rate, double *taps, int cap, int *L, int *M, int *T) {
  if (rate == 0) rate = kMpxRateIn;
  if (int rc = check_mpx_rate("fmr_mpx_output_taps", rate)) return rc;
  int l, m, t;
  std::vector<double> h;
  design_mpx_rate(rate, l, m, t, nullptr);
  if (L) *L = l;
  if (M) *M = m;
  if (T) *T = t;
  const long long n = (long long)t * l;
  if (taps && (long long)cap >= n) {
    design_mpx_rate(rate, l, m, t, &h);
    memcpy(taps, h.data(), (size_t)n * sizeof(double));
  }
  return (int)n;
}

// ---- MPX input: C-ABI ----
// cfg and in as this library knows them, from the caller's sizes
static int take_mpx_input(const char *fn, const fmr_config *cfg, size_t cfg_size, const fmr_mpx_input_config *in, size_t in_size,
                          fmr_config &full, fmr_mpx_input_config &m) {
  if (!cfg) { set_err("%s: cfg is null", fn); return FMR_ERR_BAD_ARG; }
  if (!in) { set_err("%s: in is null", fn); return FMR_ERR_BAD_ARG; }
  if (int rc = widen_config(fn, cfg, cfg_size ? cfg_size : sizeof(fmr_config), &full)) return rc;
  return take_sized(fn, "fmr_mpx_input_config", in, in_size, m);
}

int fmr_create_mpx_decoder(const fmr_config *cfg, size_t cfg_size, const fmr_mpx_input_config *in, size_t in_size, fmr_chain **out) {
  const char *fn = "fmr_create_mpx_decoder";
  if (!out) { set_err("%s: out is null", fn); return FMR_ERR_BAD_ARG; }
  *out = nullptr;
  fmr_config full;
  fmr_mpx_input_config m;
  if (int rc = take_mpx_input(fn, cfg, cfg_size, in, in_size, full, m)) return rc;
  return create_chain(&full, out, false, m.rds == 1, &m);
}

int fmr_debug_mpx_chain_shape(const fmr_config *cfg, size_t cfg_size, const fmr_mpx_input_config *in, size_t in_size,
                              fmr_chain_shape_info *out, size_t out_size) {
  const char *fn = "fmr_debug_mpx_chain_shape";
  fmr_config full;
  fmr_mpx_input_config m;
  if (int rc = take_mpx_input(fn, cfg, cfg_size, in, in_size, full, m)) return rc;
  return debug_chain_shape(fn, &full, sizeof full, 0, &m, out, out_size);
}

// what both process entry points check before anything is enqueued or any counter moves
static int check_mpx_blocks(const char *fn, fmr_chain *c, const void *pcm, const uint32_t *block_len, int n_blocks, size_t *n_frames) {
  if (!c || !pcm || !block_len || n_blocks < 1) { set_err("%s: chain, pcm or block_len is null, or n_blocks < 1", fn); return FMR_ERR_BAD_ARG; }
  if (!c->mpx_in) {
    set_err("%s: the chain takes IQ (fmr_process_blocks): only a chain made by fmr_create_mpx_decoder takes PCM frames", fn);
    return FMR_ERR_BAD_ARG;
  }
  size_t N = 0;
  for (int b = 0; b < n_blocks; b++) N += block_len[b];
  *n_frames = N;
  return FMR_OK;
}

int fmr_process_mpx_blocks_device(fmr_chain *c, const void *d_pcm, size_t stream_stride, const uint32_t *block_len,
                                  int n_blocks, double *d_audio, size_t audio_stride, uint32_t *audio_len, int sync) {
  const char *fn = "fmr_process_mpx_blocks_device";
  size_t N_in = 0;
  if (int rc = check_mpx_blocks(fn, c, d_pcm, block_len, n_blocks, &N_in)) return rc;
  try {
    if (!d_audio) { set_err("%s: d_audio is null", fn); return FMR_ERR_BAD_ARG; }
    if ((stream_stride * c->mpxi.frame_bytes()) % 16 != 0 || ((uintptr_t)d_pcm % 16) != 0) {
      set_err("%s: the PCM rows and the stream stride must be 16-byte aligned", fn);
      return FMR_ERR_BAD_ARG;
    }
    if (c->S > 1 && stream_stride < N_in) { set_err("%s: stream_stride %zu is shorter than the %zu frames of a row", fn, stream_stride, N_in); return FMR_ERR_BAD_ARG; }
    if (n_blocks <= c->max_blocks && predict_audio(c, block_len, n_blocks) > audio_stride) {
      set_err("audio_stride too small for the audio these blocks produce (nothing was processed)");
      return FMR_ERR_CAPACITY;
    }
    const int rc = c->run_cold_aware((const float2 *)d_pcm, stream_stride, block_len, n_blocks, d_audio, audio_stride, audio_len);
    if (rc) return rc;
    if (sync) return c->sync_all();
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_process_mpx_blocks(fmr_chain *c, const void *pcm, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                           double *audio, size_t audio_stride, uint32_t *audio_len) {
  const char *fn = "fmr_process_mpx_blocks";
  size_t N_in = 0;
  if (int rc = check_mpx_blocks(fn, c, pcm, block_len, n_blocks, &N_in)) return rc;
  try {
    if (N_in > c->max_in) { set_err("input longer than max_block_len*max_blocks"); return FMR_ERR_CAPACITY; }
    if (c->S > 1 && stream_stride < N_in) { set_err("%s: stream_stride %zu is shorter than the %zu frames of a row", fn, stream_stride, N_in); return FMR_ERR_BAD_ARG; }
    if (n_blocks <= c->max_blocks && audio) {
      const size_t need = predict_audio(c, block_len, n_blocks);
      if (need > audio_stride) { set_err("audio capacity %zu too small: these blocks produce %zu doubles (nothing was processed)", audio_stride, need); return FMR_ERR_CAPACITY; }
    }
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t fb = c->mpxi.frame_bytes();
    if (N_in)
      HIPCHK(hipMemcpy2DAsync(c->mpxi.d_pcm.p, fb * c->max_in, pcm, fb * stream_stride, fb * N_in, (size_t)c->S, hipMemcpyHostToDevice, c->stream));
    const size_t dstride = c->stereo ? 2 * c->max_au : c->max_au;
    std::vector<uint32_t> alen(n_blocks, 0);
    const int rc = c->run_cold_aware(reinterpret_cast<const float2 *>(c->mpxi.d_pcm.p), c->max_in, block_len, n_blocks, c->d_audio.p, dstride, alen.data());
    if (rc) return rc;
    size_t total = 0;
    for (int b = 0; b < n_blocks; b++) { total += alen[b]; if (audio_len) audio_len[b] = alen[b]; }
    if (total && audio) {
      if (total > audio_stride) { set_err("audio capacity too small"); return FMR_ERR_CAPACITY; }
      HIPCHK(hipMemcpy2DAsync(audio, sizeof(double) * audio_stride, c->d_audio.p, sizeof(double) * dstride, sizeof(double) * total, c->S,
                              hipMemcpyDeviceToHost, c->stream));
    }
    return c->sync_all();
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

int fmr_mpx_input_geometry(int rate, int *L, int *M, int *T, int *K, double *delay_samples) {
  if (rate == 0) rate = kMpxRateIn;
  if (int rc = check_mpx_rate("fmr_mpx_input_geometry", rate)) return rc;
  int l, m, t;
  design_mpx_rate(rate, l, m, t, nullptr);
  if (L) *L = l;
  if (M) *M = m;
  if (T) *T = t;
  if (K) *K = t > 1 ? mpx_in_taps_per_sample(l, m, t) : 1;
  if (delay_samples) *delay_samples = t > 1 ? ((double)t * l - 1.0) / (2.0 * l) : 0.0;
  return FMR_OK;
}

int fmr_get_mpx_input_info(fmr_chain *c, int stream, fmr_mpx_input_info *info, size_t info_size) {
  const char *fn = "fmr_get_mpx_input_info";
  if (!c || !info || stream < 0 || stream >= c->S) { set_err("%s: bad chain, info or stream", fn); return FMR_ERR_BAD_ARG; }
  if (!c->mpx_in) { set_err("%s: the chain is not an MPX decoder (fmr_create_mpx_decoder)", fn); return FMR_ERR_BAD_ARG; }
  if ((info_size ? info_size : sizeof(fmr_mpx_input_info)) > sizeof(fmr_mpx_input_info)) {
    set_err("%s: info_size %zu is larger than this library's fmr_mpx_input_info (%zu): the caller is newer than the library", fn, info_size,
            sizeof(fmr_mpx_input_info));
    return FMR_ERR_BAD_ARG;
  }
  try {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int rc = c->sync_all()) return rc;
    const MpxInStage &st = c->mpxi;
    fmr_mpx_input_info full{};
    full.struct_size = (unsigned)sizeof full;
    full.format = st.format; full.rate = c->mi_rate;
    full.L = st.geom.L; full.M = st.geom.M; full.taps_per_phase = st.geom.T; full.taps_per_sample = st.geom.K;
    full.delay_samples = st.geom.T > 1 ? ((double)st.geom.T * st.geom.L - 1.0) / (2.0 * st.geom.L) : 0.0;
    full.full_scale_hz = 75000.0 * st.gain;
    full.frames_in = st.frames; full.samples_out = st.samples;
    unsigned long long tot = 0;
    HIPCHK(hipMemcpy(&tot, st.d_tot.p + stream, sizeof tot, hipMemcpyDeviceToHost));
    full.nonfinite_in = tot;
    give_sized(info, info_size, full);
    return FMR_OK;
  } catch (const std::exception &e) { set_err("exception: %s", e.what()); return FMR_ERR_HIP; }
}

// ---- weak-signal handling: C-ABI ----
int fmr_enable_weak_signal(fmr_chain *c, const fmr_weak_signal_config *cfg, size_t cfg_size) {
  const char *fn = "fmr_enable_weak_signal";
  if (!cfg) { set_err("%s: cfg is null", fn); return FMR_ERR_BAD_ARG; }
  fmr_weak_signal_config m;
  if (int rc = take_sized(fn, "fmr_weak_signal_config", cfg, cfg_size, m)) return rc;
  if (m.mode != FMR_WS_MEASURE && m.mode != FMR_WS_ACT) {
    set_err("%s: mode %d is neither FMR_WS_MEASURE (0) nor FMR_WS_ACT (1)", fn, m.mode);
    return FMR_ERR_BAD_ARG;
  }
  if (m.actions == 0) m.actions = FMR_WS_BLEND | FMR_WS_HIGHCUT | FMR_WS_MUTE;
  if (m.actions & ~7u) { set_err("%s: actions 0x%x has bits beyond FMR_WS_BLEND | FMR_WS_HIGHCUT | FMR_WS_MUTE", fn, m.actions); return FMR_ERR_BAD_ARG; }
  if (int rc = check_field(fn, "record_intervals", m.record_intervals, 1, 1000, 50)) return rc;
  if (int rc = check_field(fn, "max_records", m.max_records, 1, 65536, 1024)) return rc;
  if (m.attack_ms == 0.0) m.attack_ms = 10.0;
  if (m.release_ms == 0.0) m.release_ms = 500.0;
  if (!(m.attack_ms > 0.0 && m.attack_ms <= 60000.0)) { set_err("%s: attack_ms %g is outside (0, 60000] (0 = 10)", fn, m.attack_ms); return FMR_ERR_BAD_ARG; }
  if (!(m.release_ms > 0.0 && m.release_ms <= 60000.0)) { set_err("%s: release_ms %g is outside (0, 60000] (0 = 500)", fn, m.release_ms); return FMR_ERR_BAD_ARG; }
  struct Pair { const char *name; double *lo, *hi; double dlo, dhi; };
  const Pair pairs[3] = {{"blend", &m.blend_lo_db, &m.blend_hi_db, kWsBlendLo, kWsBlendHi},
                         {"highcut", &m.highcut_lo_db, &m.highcut_hi_db, kWsBlendHi, kWsHighcutHi},
                         {"mute", &m.mute_lo_db, &m.mute_hi_db, kWsHighcutHi, kWsMuteHi}};
  for (const Pair &p : pairs) {
    if (*p.lo == 0.0 && *p.hi == 0.0) { *p.lo = p.dlo; *p.hi = p.dhi; }
    if (!(std::isfinite(*p.lo) && std::isfinite(*p.hi) && *p.lo < *p.hi)) {
      set_err("%s: %s_lo_db %g and %s_hi_db %g are not finite with lo < hi (both 0 = %g and %g)", fn, p.name, *p.lo, p.name, *p.hi, p.dlo, p.dhi);
      return FMR_ERR_BAD_ARG;
    }
  }
  if (int rc = check_field(fn, "highcut_hz", m.highcut_hz, 500.0, 15000.0, 2500.0)) return rc;
  if (m.mute_floor_db == 0.0) m.mute_floor_db = -20.0;
  if (!(std::isfinite(m.mute_floor_db) && m.mute_floor_db < 0.0)) { set_err("%s: mute_floor_db %g is not finite and below 0 (0 = -20)", fn, m.mute_floor_db); return FMR_ERR_BAD_ARG; }
  if (!c) { set_err("%s: chain is null", fn); return FMR_ERR_BAD_ARG; }
  if (c->mode != FMR_MODE_FM) {
    set_err("%s: weak-signal handling reads the MPX of an FM chain (mode FMR_MODE_FM); mode %d %s", fn, c->mode,
            c->mode == FMR_MODE_NONE ? "is a front-end-only chain (channelizer / IfResampler): it has no MPX" : "is not covered");
    return FMR_ERR_UNSUPPORTED;
  }
  if (c->pilot_shift) {
    set_err("%s: the chain has pilot_shift (the QMM output): its two channels are not L and R", fn);
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage(fn, c, c->ws, "weak-signal stage", "MPX sample", c->S, c->max_if, c->max_au, m);
}

int fmr_weak_signal_read(fmr_chain *c, int stream, fmr_weak_signal_record *recs, int cap, fmr_weak_signal_info *info,
                         size_t info_size) {
  return read_records("fmr_weak_signal_read", c, &fmr_chain::ws, "weak-signal stage", "fmr_enable_weak_signal", stream, recs, cap, info,
                      info_size, copy_ring(recs), nullptr, [c](fmr_weak_signal_info &full, const WeakSignalStage &ws) {
    full.channels = c->stereo ? 2 : 1;
    full.intervals_complete = ws.intervals();
    full.record_intervals = ws.cfg.record_intervals;
    full.max_records = ws.cfg.max_records;
    full.mode = ws.cfg.mode;
    full.actions = ws.cfg.actions;
  });
}

int fmr_weak_signal_derive(const fmr_weak_signal_record *recs, int n, fmr_weak_signal_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_weak_signal_derive", recs && out, "recs or out", n)) return rc;
  if (int rc = derive_intervals("fmr_weak_signal_derive", "fmr_weak_signal_read", recs, n)) return rc;
  fmr_weak_signal_levels full{};
  full.struct_size = (unsigned)sizeof full;
  double sum = 0.0, peak = 0.0;
  unsigned long long ni = 0, nb = 0, nh = 0, nm = 0, non = 0;
  for (int i = 0; i < n; i++) {
    const fmr_weak_signal_record &r = recs[i];
    sum += r.usn_sum;
    peak = std::max(peak, r.usn_peak);
    ni += r.n_intervals; non += r.n_nonfinite;
    if (r.max_blend > 0.0) nb += r.n_intervals;
    if (r.max_highcut > 0.0) nh += r.n_intervals;
    if (r.max_mute > 0.0) nm += r.n_intervals;
  }
  const double mean = sum / (double)ni;
  full.usn_mean_db = db10(mean); full.usn_peak_db = db10(peak);
  full.usn_mean_hz = 75000.0 * std::sqrt(mean); full.usn_peak_hz = 75000.0 * std::sqrt(peak);
  full.blend_share = (double)nb / (double)ni; full.highcut_share = (double)nh / (double)ni; full.mute_share = (double)nm / (double)ni;
  full.t_blend = recs[n - 1].t_blend; full.t_highcut = recs[n - 1].t_highcut; full.t_mute = recs[n - 1].t_mute;
  full.n_intervals = ni; full.n_nonfinite = non;
  give_sized(out, out_size, full);
  return FMR_OK;
}

// ---- impulse blanker: C-ABI ----
int fmr_enable_blanker(fmr_chain *c, const fmr_blanker_config *cfg, size_t cfg_size) {
  const char *fn = "fmr_enable_blanker";
  if (!cfg) { set_err("%s: cfg is null", fn); return FMR_ERR_BAD_ARG; }
  fmr_blanker_config m;
  if (int rc = take_sized(fn, "fmr_blanker_config", cfg, cfg_size, m)) return rc;
  if (m.mode != FMR_NB_MEASURE && m.mode != FMR_NB_ACT) {
    set_err("%s: mode %d is neither FMR_NB_MEASURE (0) nor FMR_NB_ACT (1)", fn, m.mode);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field(fn, "threshold_db", m.threshold_db, 6.0, 40.0, 12.0)) return rc;
  if (m.gate_samples < 0 || m.gate_samples > kNbMaxG) {
    set_err("%s: gate_samples %d is outside 1 .. %d (0 = max(2, ceil(0.8e-6 input_rate)))", fn, m.gate_samples, kNbMaxG);
    return FMR_ERR_BAD_ARG;
  }
  auto bad_run = [&](int G) {
    set_err("%s: max_run_samples %d is outside gate_samples (%d) .. %d (0 = 8 gate_samples, %d at most)", fn, m.max_run_samples, G, kNbMaxM, kNbMaxM);
    return FMR_ERR_BAD_ARG;
  };
  if (m.max_run_samples < 0 || m.max_run_samples > kNbMaxM || (m.max_run_samples && m.max_run_samples < std::max(1, m.gate_samples)))
    return bad_run(std::max(1, m.gate_samples));
  if (int rc = check_field(fn, "average_intervals", m.average_intervals, 1, kNbMaxW, 16)) return rc;
  if (int rc = check_field(fn, "record_intervals", m.record_intervals, 1, 4096, 256)) return rc;
  if (int rc = check_field(fn, "max_records", m.max_records, 1, 65536, 1024)) return rc;
  if (!c) { set_err("%s: chain is null", fn); return FMR_ERR_BAD_ARG; }
  if (int rc = refuse_no_capture(fn, c, "the blanker")) return rc;
  // (the gate is a time, 0.8 us: longer than an impulse, shorter than one IF sample)
  if (m.gate_samples == 0) m.gate_samples = std::min(kNbMaxG, std::max(2, (int)std::ceil(0.8e-6 * c->cfg.input_rate)));
  if (m.max_run_samples == 0) m.max_run_samples = std::min(kNbMaxM, 8 * m.gate_samples);
  if (m.max_run_samples < m.gate_samples) return bad_run(m.gate_samples);
  static_assert(kNbMaxG - 1 + kNbMaxM <= kNbQ, "G - 1 + M <= Q holds for every accepted G and M");
  return enable_stage(fn, c, c->nb, "blanker", "input sample", c->in_rows(), c->max_in, m);
}

int fmr_blanker_read(fmr_chain *c, int row, fmr_blanker_record *recs, int cap, fmr_blanker_info *info, size_t info_size) {
  return read_records("fmr_blanker_read", c, &fmr_chain::nb, "blanker", "fmr_enable_blanker", row, recs, cap, info, info_size,
                      copy_ring(recs), nullptr, [](fmr_blanker_info &full, const BlankerStage &nb) {
    const fmr_blanker_config &m = nb.cfg;
    full.rows = nb.rows;
    full.intervals_complete = nb.intervals();
    full.mode = m.mode; full.gate_samples = m.gate_samples; full.max_run_samples = m.max_run_samples;
    full.average_intervals = m.average_intervals; full.record_intervals = m.record_intervals; full.max_records = m.max_records;
  });
}

int fmr_blanker_derive(const fmr_blanker_record *recs, int n, double input_rate, fmr_blanker_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_blanker_derive", recs && out, "recs or out", n)) return rc;
  if (!(input_rate > 0.0) || !std::isfinite(input_rate)) { set_err("fmr_blanker_derive: input_rate %g is not a positive rate", input_rate); return FMR_ERR_BAD_ARG; }
  if (int rc = derive_intervals("fmr_blanker_derive", "fmr_blanker_read", recs, n)) return rc;
  fmr_blanker_levels full{};
  full.struct_size = (unsigned)sizeof full;
  double pq = 0.0;
  float peak = 0.f;
  for (int i = 0; i < n; i++) {
    const fmr_blanker_record &r = recs[i];
    full.n_intervals += r.n_intervals; full.n_triggers += r.n_triggers; full.n_blanked += r.n_blanked;
    full.n_nonfinite += r.n_nonfinite; full.n_runs += r.n_runs;
    pq += (double)r.power_q;
    peak = std::max(peak, r.peak);
  }
  const double samples = (double)full.n_intervals * (double)kNbQ;
  full.blanked_share = (double)full.n_blanked / samples;
  full.runs_per_second = (double)full.n_runs * input_rate / samples;
  full.level_dbfs = db10(pq / ((double)full.n_intervals * 68719476736.0));
  full.peak_dbfs = db10((double)peak);
  give_sized(out, out_size, full);
  return FMR_OK;
}

// ---- IQ correction: C-ABI ----
int fmr_enable_iq_correction(fmr_chain *c, const fmr_iq_correction_config *cfg, size_t cfg_size) {
  const char *fn = "fmr_enable_iq_correction";
  if (!cfg) { set_err("%s: cfg is null", fn); return FMR_ERR_BAD_ARG; }
  fmr_iq_correction_config m;
  if (int rc = take_sized(fn, "fmr_iq_correction_config", cfg, cfg_size, m)) return rc;
  if (m.mode != FMR_IQC_MEASURE && m.mode != FMR_IQC_ACT) {
    set_err("%s: mode %d is neither FMR_IQC_MEASURE (0) nor FMR_IQC_ACT (1)", fn, m.mode);
    return FMR_ERR_BAD_ARG;
  }
  if (m.correct == 0) m.correct = FMR_IQC_DC | FMR_IQC_BALANCE;
  if (m.correct < 0 || m.correct > (FMR_IQC_DC | FMR_IQC_BALANCE)) {
    set_err("%s: correct %d is not a mask of FMR_IQC_DC (1) and FMR_IQC_BALANCE (2) (0 = both)", fn, m.correct);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field(fn, "average_intervals", m.average_intervals, 1, kIqcMaxW, 64)) return rc;
  if (int rc = check_field(fn, "record_intervals", m.record_intervals, 1, 4096, 256)) return rc;
  if (int rc = check_field(fn, "max_records", m.max_records, 1, 65536, 1024)) return rc;
  if (!c) { set_err("%s: chain is null", fn); return FMR_ERR_BAD_ARG; }
  if (int rc = refuse_no_capture(fn, c, "the IQ corrector")) return rc;
  return enable_stage(fn, c, c->iqc, "IQ corrector", "input sample", c->in_rows(), c->max_in, m);
}

int fmr_iq_correction_read(fmr_chain *c, int row, fmr_iq_correction_record *recs, int cap, fmr_iq_correction_info *info,
                           size_t info_size) {
  return read_records("fmr_iq_correction_read", c, &fmr_chain::iqc, "IQ corrector", "fmr_enable_iq_correction", row, recs, cap, info,
                      info_size, copy_ring(recs), nullptr, [](fmr_iq_correction_info &full, const IqCorrectionStage &iqc) {
    const fmr_iq_correction_config &m = iqc.cfg;
    full.rows = iqc.rows;
    full.intervals_complete = iqc.intervals();
    full.mode = m.mode; full.correct = m.correct; full.average_intervals = m.average_intervals;
    full.record_intervals = m.record_intervals; full.max_records = m.max_records;
  });
}

int fmr_iq_correction_derive(const fmr_iq_correction_record *recs, int n, fmr_iq_correction_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_iq_correction_derive", recs && out, "recs or out", n)) return rc;
  if (int rc = derive_intervals("fmr_iq_correction_derive", "fmr_iq_correction_read", recs, n)) return rc;
  fmr_iq_correction_levels full{};
  full.struct_size = (unsigned)sizeof full;
  int64_t S_r = 0, S_i = 0, S_rr = 0, S_ii = 0, S_ri = 0;
  for (int i = 0; i < n; i++) {
    const fmr_iq_correction_record &r = recs[i];
    full.n_intervals += r.n_intervals; full.n_usable += r.n_usable; full.n_nonfinite += r.n_nonfinite;
    full.n_skipped += r.n_skipped; full.n_refused += r.n_refused;
    S_r += r.sum_re; S_i += r.sum_im; S_rr += r.sum_rr; S_ii += r.sum_ii; S_ri += r.sum_ri;
  }
  full.usable_share = (double)full.n_usable / ((double)full.n_intervals * (double)kNbQ);
  double w_r = 0.0, w_i = 0.0;
  if (full.n_usable >= (uint64_t)(kNbQ / 2)) {       // the header's formulas, operation by operation
    const double r = 1.0 / ((double)full.n_usable * 68719476736.0);
    const double m_r = (double)S_r * r, m_i = (double)S_i * r;
    const double E_rr = (double)S_rr * r, E_ii = (double)S_ii * r, E_ri = (double)S_ri * r;
    const double P = (E_rr + E_ii) - (m_r * m_r + m_i * m_i);
    const double C_r = (E_rr - E_ii) - (m_r * m_r - m_i * m_i);
    const double C_i = 2.0 * E_ri - 2.0 * (m_r * m_i);
    const double D = P * P - (C_r * C_r + C_i * C_i);
    if (P > 9.094947017729282e-13 && D > 0.0) {
      const double t = P + std::sqrt(D);
      w_r = C_r / t; w_i = C_i / t;
      if (w_r * w_r + w_i * w_i > 0.0625) { w_r = 0.0; w_i = 0.0; full.refused = 1; }
    }
    full.dc_re = m_r; full.dc_im = m_i;
  }
  full.w_re = w_r; full.w_im = w_i;
  const double ad = std::hypot(full.dc_re, full.dc_im), aw = std::hypot(w_r, w_i);
  full.dc_dbfs = ad > 0.0 ? 20.0 * std::log10(ad) : -INFINITY;
  full.image_rejection_db = aw > 0.0 ? -20.0 * std::log10(aw) : INFINITY;
  const std::complex<double> rho = (1.0 - std::complex<double>(w_r, w_i)) / (1.0 + std::complex<double>(w_r, w_i));
  full.gain_imbalance_db = 20.0 * std::log10(std::abs(rho));
  full.phase_error_deg = -std::arg(rho) * (180.0 / 3.14159265358979323846);
  give_sized(out, out_size, full);
  return FMR_OK;
}

// ---- audio monitor: C-ABI ----
int fmr_enable_loudness(fmr_chain *c, const fmr_loudness_config *cfg, size_t cfg_size) {
  if (!cfg) { set_err("fmr_enable_loudness: cfg is null"); return FMR_ERR_BAD_ARG; }
  fmr_loudness_config m;
  if (int rc = take_sized("fmr_enable_loudness", "fmr_loudness_config", cfg, cfg_size, m)) return rc;
  if (m.step_samples == 0) m.step_samples = 4800;
  if (m.step_samples % 16 != 0 || m.step_samples < 48 || m.step_samples > (1u << 20)) {
    set_err("fmr_enable_loudness: step_samples %u is not a multiple of 16 in 48 .. 2^20 (0 = 4800)", m.step_samples);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field("fmr_enable_loudness", "max_records", m.max_records, 1, 65536, 1024)) return rc;
  if (!c) { set_err("fmr_enable_loudness: chain is null"); return FMR_ERR_BAD_ARG; }
  if (c->mode != FMR_MODE_FM) {
    set_err("fmr_enable_loudness: the audio monitor reads the audio of an FM chain (mode FMR_MODE_FM); mode %d %s", c->mode,
            c->mode == FMR_MODE_NONE ? "is a front-end-only chain (channelizer / IfResampler): it has no audio" : "is not covered");
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage("fmr_enable_loudness", c, c->ld, "audio monitor", "audio sample", c->S, c->max_au, m);
}

int fmr_loudness_read(fmr_chain *c, int stream, fmr_loudness_record *recs, int cap, fmr_loudness_info *info, size_t info_size) {
  return read_records("fmr_loudness_read", c, &fmr_chain::ld, "audio monitor", "fmr_enable_loudness", stream, recs, cap, info, info_size,
                      copy_ring(recs), nullptr, [c](fmr_loudness_info &full, const LoudnessStage &ld) {
    full.channels = c->stereo ? 2 : 1;
    full.step_samples = ld.cfg.step_samples;
    full.max_records = ld.cfg.max_records;
  });
}

int fmr_loudness_derive(const fmr_loudness_record *recs, int n, double silence_dbfs, fmr_loudness_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_loudness_derive", recs && out, "recs or out", n)) return rc;
  if (std::isnan(silence_dbfs)) { set_err("fmr_loudness_derive: silence_dbfs is not a number"); return FMR_ERR_BAD_ARG; }
  for (int i = 0; i < n; i++)
    if (recs[i].step_samples == 0 || recs[i].channels < 1 || recs[i].channels > 2) {
      set_err("fmr_loudness_derive: record %d has step_samples %u and channels %u (not a record of fmr_loudness_read)", i,
              recs[i].step_samples, recs[i].channels);
      return FMR_ERR_BAD_ARG;
    }
  auto lufs = [](double z) { return z > 0.0 ? -0.691 + 10.0 * std::log10(z) : -INFINITY; };
  auto db20 = [](double v) { return v > 0.0 ? 20.0 * std::log10(v) : -INFINITY; };
  fmr_loudness_levels full{};
  full.struct_size = (unsigned)sizeof full;
  full.momentary_lufs = full.momentary_max_lufs = full.short_term_lufs = full.short_term_max_lufs = -INFINITY;
  std::vector<double> zm;            // the mean squares of all momentary windows
  double sl = 0.0, sr = 0.0, slr = 0.0, sp = 0.0, tp = 0.0;
  unsigned long long run = 0;        // silent records that end at i
  const double thr = std::pow(10.0, silence_dbfs / 10.0);
  int consec = 0;                    // records with consecutive index that end at i
  for (int i = 0; i < n; i++) {
    const fmr_loudness_record &r = recs[i];
    const bool follows = i > 0 && r.index == recs[i - 1].index + 1;
    consec = follows ? consec + 1 : 1;
    if (!follows) run = 0;
    const double Q = (double)r.step_samples;
    sl += r.sumsq[0]; sr += r.sumsq[1]; slr += r.sum_lr;
    sp = std::max(sp, std::max(r.sample_peak[0], r.sample_peak[1]));
    tp = std::max(tp, std::max(r.true_peak[0], r.true_peak[1]));
    full.n_nonfinite += r.n_nonfinite;
    auto window = [&](int w) {       // the K-weighted mean square of the records i - w + 1 .. i, channels added
      double z = 0.0;
      for (int j = i - w + 1; j <= i; j++) z += recs[j].kw_sumsq[0] + recs[j].kw_sumsq[1];
      return z / ((double)w * Q);
    };
    if (consec >= 4) {
      const double z = window(4);
      zm.push_back(z);
      full.momentary_lufs = lufs(z);
      full.momentary_max_lufs = std::max(full.momentary_max_lufs, full.momentary_lufs);
    }
    if (consec >= 30) {
      full.short_term_lufs = lufs(window(30));
      full.short_term_max_lufs = std::max(full.short_term_max_lufs, full.short_term_lufs);
    }
    run = (r.sumsq[0] + r.sumsq[1]) / ((double)r.channels * Q) < thr ? run + 1 : 0;
    full.longest_silence_blocks = std::max<uint64_t>(full.longest_silence_blocks, run);
  }
  full.trailing_silence_blocks = run;
  // BS.1770-4 gating over the momentary windows: -70 LUFS absolute, then 10 LU under the mean of what passed
  full.momentary_windows = zm.size();
  full.integrated_lufs = -INFINITY;
  double za = 0.0;
  size_t na = 0;
  for (double z : zm) if (lufs(z) > -70.0) { za += z; na++; }
  if (na > 0) {
    const double gate = lufs(za / (double)na) - 10.0;
    double zg = 0.0;
    size_t ng = 0;
    for (double z : zm) if (lufs(z) > -70.0 && lufs(z) > gate) { zg += z; ng++; }
    full.gated_windows = ng;
    if (ng > 0) full.integrated_lufs = lufs(zg / (double)ng);
  }
  full.sample_peak_dbfs = db20(sp);
  full.true_peak_dbtp = db20(tp);
  const double den = sl * sr;
  full.correlation = den > 0.0 ? slr / std::sqrt(den) : 0.0;
  const double side = sl + sr - 2.0 * slr, mid = sl + sr + 2.0 * slr;
  full.side_to_mid_db = side <= 0.0 && mid <= 0.0 ? 0.0 : side <= 0.0 ? -INFINITY : mid <= 0.0 ? INFINITY : 10.0 * std::log10(side / mid);
  give_sized(out, out_size, full);
  return FMR_OK;
}

// ---- audio analyser: C-ABI ----
int fmr_enable_analyser(fmr_chain *c, const fmr_analyser_config *cfg, size_t cfg_size) {
  if (!cfg) { set_err("fmr_enable_analyser: cfg is null"); return FMR_ERR_BAD_ARG; }
  fmr_analyser_config m;
  if (int rc = take_sized("fmr_enable_analyser", "fmr_analyser_config", cfg, cfg_size, m)) return rc;
  if (m.fft_size == 0) m.fft_size = 4096;
  if (m.fft_size != 1024 && m.fft_size != 2048 && m.fft_size != 4096 && m.fft_size != 8192) {
    set_err("fmr_enable_analyser: fft_size %d is not 1024, 2048, 4096 or 8192 (0 = 4096)", m.fft_size);
    return FMR_ERR_BAD_ARG;
  }
  const uint32_t H = (uint32_t)m.fft_size / 2;
  if (m.interval_samples == 0) m.interval_samples = 6u * (uint32_t)m.fft_size;
  if (m.interval_samples % H != 0 || m.interval_samples < H || m.interval_samples > (1u << 24)) {
    set_err("fmr_enable_analyser: interval_samples %u is not a multiple of fft_size / 2 = %u in %u .. 2^24 (0 = 6 fft_size)",
            m.interval_samples, H, H);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field("fmr_enable_analyser", "max_records", m.max_records, 1, 4096, 64)) return rc;
  if (!c) { set_err("fmr_enable_analyser: chain is null"); return FMR_ERR_BAD_ARG; }
  if (!c->has_dec) {
    set_err("fmr_enable_analyser: a front-end-only chain (mode -1: channelizer / IfResampler) has no audio");
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage("fmr_enable_analyser", c, c->an, "analyser", "audio sample", c->S, c->max_au, m);
}

int fmr_analyser_read(fmr_chain *c, int stream, fmr_analyser_record *recs, double *spectra, int cap, fmr_analyser_info *info,
                      size_t info_size) {
  return read_records(
      "fmr_analyser_read", c, &fmr_chain::an, "analyser", "fmr_enable_analyser", stream, recs, cap, info, info_size,
      [=](AnalyserStage &an, size_t k, size_t at, size_t m) -> int {
        const size_t nb3 = (size_t)kAnRows * (size_t)an.nb;
        HIPCHK(hipMemcpy(recs + k, an.d_ring_rec.p + at, m * sizeof(fmr_analyser_record), hipMemcpyDeviceToHost));
        if (spectra) HIPCHK(hipMemcpy(spectra + k * nb3, an.d_ring_psd.p + at * nb3, m * nb3 * sizeof(double), hipMemcpyDeviceToHost));
        return FMR_OK;
      },
      [=](const AnalyserStage &an, int n) {      // the sums of the counted segments -> power
        if (!spectra || cap == 0) return;
        const size_t nb = (size_t)an.nb, nb3 = (size_t)kAnRows * nb;
        for (int i = 0; i < n; i++) {
          const double seg = (double)recs[i].segments;
          const double g = seg > 0.0 ? 1.0 / ((double)an.N * an.sumw2 * seg) : 0.0;
          for (int r = 0; r < kAnRows; r++) {
            double *row = spectra + (size_t)i * nb3 + (size_t)r * nb;
            for (size_t k = 0; k < nb; k++) row[k] = row[k] * ((k == 0 || k == nb - 1) ? 1.0 : 2.0) * g;
          }
        }
      },
      [c](fmr_analyser_info &full, const AnalyserStage &an) {
        full.channels = c->stereo ? 2 : 1;
        full.interval_samples = an.cfg.interval_samples;
        full.max_records = an.cfg.max_records;
        full.fft_size = an.N;
        full.bins = an.nb;
        full.bin_hz = kPcmRate / an.N;
      });
}

int fmr_analyser_derive(const fmr_analyser_record *recs, const double *spectra, int n, const fmr_analyser_rule *rule,
                        size_t rule_size, fmr_analyser_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_analyser_derive", recs && spectra && out, "recs, spectra or out", n)) return rc;
  fmr_analyser_rule r{};
  if (rule) if (int rc = take_sized("fmr_analyser_derive", "fmr_analyser_rule", rule, rule_size, r)) return rc;
  const int N = (int)recs[0].fft_size, ch = (int)recs[0].channels;
  if ((N != 1024 && N != 2048 && N != 4096 && N != 8192) || ch < 1 || ch > 2) {
    set_err("fmr_analyser_derive: record 0 has fft_size %d and channels %d (not a record of fmr_analyser_read)", N, ch);
    return FMR_ERR_BAD_ARG;
  }
  for (int i = 1; i < n; i++)
    if ((int)recs[i].fft_size != N || (int)recs[i].channels != ch) {
      set_err("fmr_analyser_derive: record %d has fft_size %u and channels %u, record 0 has %d and %d", i, recs[i].fft_size,
              recs[i].channels, N, ch);
      return FMR_ERR_BAD_ARG;
    }
  if (r.view < 0 || r.view > 3 || (ch == 1 && r.view != 0)) {
    set_err("fmr_analyser_derive: view %d is not 0 .. 3 (0 only for records of one channel; these have %d)", r.view, ch);
    return FMR_ERR_BAD_ARG;
  }
  if (r.band_lo_hz == 0.0) r.band_lo_hz = 20.0;
  if (r.band_hi_hz == 0.0) r.band_hi_hz = 15000.0;
  if (r.tone_search_hz == 0.0) r.tone_search_hz = 50.0;
  if (r.max_harmonic == 0) r.max_harmonic = 10;
  if (r.min_tone_dbfs == 0.0) r.min_tone_dbfs = -60.0;
  constexpr int W = 4;
  const double bin_hz = kPcmRate / N;
  if (!(r.band_lo_hz >= 0.0) || !(r.band_hi_hz <= kPcmRate / 2) || !(r.band_lo_hz < r.band_hi_hz)) {
    set_err("fmr_analyser_derive: band_lo_hz %g and band_hi_hz %g are not 0 <= lo < hi <= 24000 (0 = 20 and 15000)", r.band_lo_hz,
            r.band_hi_hz);
    return FMR_ERR_BAD_ARG;
  }
  const int k_lo = (int)std::ceil(r.band_lo_hz / bin_hz), k_hi = (int)std::floor(r.band_hi_hz / bin_hz);
  const int B = k_hi - k_lo + 1;
  if (B < 2 * W + 1) {
    set_err("fmr_analyser_derive: band_lo_hz %g .. band_hi_hz %g holds %d bins of %g Hz, fewer than %d", r.band_lo_hz, r.band_hi_hz,
            B, bin_hz, 2 * W + 1);
    return FMR_ERR_BAD_ARG;
  }
  if (!(r.tone_hz >= 0.0) || !(r.tone_hz <= kPcmRate / 2)) {
    set_err("fmr_analyser_derive: tone_hz %g is outside 0 .. 24000 (0 = the strongest bin)", r.tone_hz);
    return FMR_ERR_BAD_ARG;
  }
  if (!(r.tone_search_hz > 0.0) || !std::isfinite(r.tone_search_hz)) {
    set_err("fmr_analyser_derive: tone_search_hz %g is not a finite value > 0 (0 = 50)", r.tone_search_hz);
    return FMR_ERR_BAD_ARG;
  }
  if (r.max_harmonic < 2 || r.max_harmonic > 64) {
    set_err("fmr_analyser_derive: max_harmonic %d is outside 2 .. 64 (0 = 10)", r.max_harmonic);
    return FMR_ERR_BAD_ARG;
  }
  if (r.reserved != 0) { set_err("fmr_analyser_derive: reserved is %d, not 0", r.reserved); return FMR_ERR_BAD_ARG; }
  if (std::isnan(r.min_tone_dbfs)) { set_err("fmr_analyser_derive: min_tone_dbfs is not a number"); return FMR_ERR_BAD_ARG; }

  // the pooled view
  const size_t nb = (size_t)N / 2 + 1, nb3 = 3 * nb;
  fmr_analyser_levels full{};
  full.struct_size = (unsigned)sizeof full;
  double seg = 0.0, s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
  for (int i = 0; i < n; i++) {
    seg += (double)recs[i].segments;
    full.segments += recs[i].segments; full.skipped += recs[i].skipped; full.n_nonfinite += recs[i].n_nonfinite;
    s0 += recs[i].sum[0]; s1 += recs[i].sum[1]; q0 += recs[i].sumsq[0]; q1 += recs[i].sumsq[1];
  }
  std::vector<double> P(nb, 0.0);
  for (size_t k = 0; k < nb; k++) {
    double pl = 0.0, pr = 0.0, pc = 0.0;
    for (int i = 0; i < n; i++) {
      const double w = (double)recs[i].segments;
      const double *sp = spectra + (size_t)i * nb3;
      pl += w * sp[k]; pr += w * sp[nb + k]; pc += w * sp[2 * nb + k];
    }
    if (seg > 0.0) { pl /= seg; pr /= seg; pc /= seg; }
    P[k] = r.view == 0 ? pl : r.view == 1 ? pr : r.view == 2 ? (pl + pr + 2.0 * pc) / 4.0 : std::max(0.0, (pl + pr - 2.0 * pc) / 4.0);
  }
  auto db = [](double p) { return p > 0.0 ? 10.0 * std::log10(2.0 * p) : -INFINITY; };
  const double frames = (double)(full.segments + full.skipped) * (double)(N / 2);
  const double sv = r.view == 0 ? s0 : r.view == 1 ? s1 : r.view == 2 ? (s0 + s1) / 2.0 : (s0 - s1) / 2.0;
  full.dc = frames > 0.0 ? sv / frames : 0.0;
  full.total_dbfs = r.view >= 2 ? NAN : frames > 0.0 ? db((r.view == 0 ? q0 : q1) / frames) : -INFINITY;
  double p_band = 0.0;
  for (int k = k_lo; k <= k_hi; k++) p_band += P[k];
  full.band_dbfs = db(p_band);

  // the tone
  int s_lo = k_lo, s_hi = k_hi;
  if (r.tone_hz > 0.0) {
    s_lo = std::max(k_lo, (int)std::ceil((r.tone_hz - r.tone_search_hz) / bin_hz));
    s_hi = std::min(k_hi, (int)std::floor((r.tone_hz + r.tone_search_hz) / bin_hz));
  }
  int k0 = -1;
  for (int k = s_lo; k <= s_hi; k++)
    if (k0 < 0 || P[k] > P[k0]) k0 = k;
  double p_t = 0.0, cen = 0.0;
  if (k0 >= 0) {
    k0 = std::min(std::max(k0, k_lo + W), k_hi - W);
    for (int k = k0 - W; k <= k0 + W; k++) { p_t += P[k]; cen += (double)k * P[k]; }
  }
  const bool found = k0 >= 2 * W + 1 && p_t > 0.0 && db(p_t) >= r.min_tone_dbfs;
  full.tone_found = found ? 1 : 0;
  for (double &h : full.harmonic_dbc) h = NAN;
  if (!found) {
    full.tone_hz = full.tone_dbfs = full.thd = full.thd_n = full.sinad_db = NAN;
    full.noise_dbfs = full.band_dbfs;
    give_sized(out, out_size, full);
    return FMR_OK;
  }
  full.tone_hz = cen / p_t * bin_hz;
  full.tone_dbfs = db(p_t);
  std::vector<char> taken(nb, 0);
  int E = 0;
  for (int k = k0 - W; k <= k0 + W; k++) { taken[k] = 1; E++; }
  double p_h = 0.0;
  for (int h = 2; h <= r.max_harmonic; h++) {
    const int kh = (int)std::floor((double)h * full.tone_hz / bin_hz + 0.5);
    if (kh + W > k_hi) break;
    double ph = 0.0;
    for (int k = kh - W; k <= kh + W; k++)
      if (!taken[k]) { ph += P[k]; taken[k] = 1; E++; }
    p_h += ph;
    full.harmonics_counted++;
    if (h <= 9) full.harmonic_dbc[h - 2] = ph > 0.0 ? 10.0 * std::log10(ph / p_t) : -INFINITY;
  }
  double p_free = 0.0;               // = P_band - P_t - P_h, without the cancellation
  for (int k = k_lo; k <= k_hi; k++)
    if (!taken[k]) p_free += P[k];
  const double p_n = B > E ? p_free * (double)B / (double)(B - E) : 0.0;
  full.noise_dbfs = db(p_n);
  full.thd = std::sqrt(p_h / p_t);
  full.thd_n = std::sqrt((p_h + p_n) / p_t);
  full.sinad_db = p_h + p_n > 0.0 ? 10.0 * std::log10((p_t + p_h + p_n) / (p_h + p_n)) : INFINITY;
  give_sized(out, out_size, full);
  return FMR_OK;
}

// ---- RF monitor: C-ABI ----
int fmr_enable_rf_monitor(fmr_chain *c, const fmr_rf_monitor_config *cfg, size_t cfg_size) {
  if (!cfg) { set_err("fmr_enable_rf_monitor: cfg is null"); return FMR_ERR_BAD_ARG; }
  fmr_rf_monitor_config m;
  if (int rc = take_sized("fmr_enable_rf_monitor", "fmr_rf_monitor_config", cfg, cfg_size, m)) return rc;
  if (m.interval_samples == 0) m.interval_samples = 38400;
  if (m.interval_samples % kMonH != 0 || m.interval_samples < (uint32_t)kMonH || m.interval_samples > (1u << 30)) {
    set_err("fmr_enable_rf_monitor: interval_samples %u is not a multiple of 512 in 512 .. 2^30 (0 = 38400)", m.interval_samples);
    return FMR_ERR_BAD_ARG;
  }
  if (int rc = check_field("fmr_enable_rf_monitor", "max_records", m.max_records, 1, 4096, 64)) return rc;
  if (!c) { set_err("fmr_enable_rf_monitor: chain is null"); return FMR_ERR_BAD_ARG; }
  if (c->mpx_in) {
    set_err("fmr_enable_rf_monitor: the RF monitor reads the IF samples in front of the discriminator; an MPX decoder (fmr_create_mpx_decoder) is fed composite PCM and has none");
    return FMR_ERR_UNSUPPORTED;
  }
  if (c->mode != FMR_MODE_FM) {
    set_err("fmr_enable_rf_monitor: the RF monitor reads the decoder input of an FM chain (mode FMR_MODE_FM); mode %d %s", c->mode,
            c->mode == FMR_MODE_NONE ? "is a front-end-only chain (channelizer / IfResampler): it has no decoder" : "is not measured");
    return FMR_ERR_UNSUPPORTED;
  }
  return enable_stage("fmr_enable_rf_monitor", c, c->rfm, "RF monitor", "IF sample", c->S, c->max_if, m.interval_samples, kRfmBins,
                      0.0, m.max_records);
}

int fmr_rf_monitor_read(fmr_chain *c, int stream, fmr_rf_monitor_record *recs, uint32_t *hist, double *psd, int cap,
                        fmr_rf_monitor_info *info, size_t info_size) {
  return read_records("fmr_rf_monitor_read", c, &fmr_chain::rfm, "RF monitor", "fmr_enable_rf_monitor", stream, recs, cap, info,
                      info_size, copy_seg_monitor(recs, hist, psd), nullptr, [](fmr_rf_monitor_info &full, const SegMonitor &m) {
    full.hist_bins = kRfmBins;
    full.psd_bins = kMonPsd;
    full.interval_samples = m.interval;
    full.max_records = (int)m.cur.L;
    full.bin_hz = kFmRate / kMonN;
  });
}

int fmr_rf_monitor_derive(const fmr_rf_monitor_record *recs, const uint32_t *hist, const double *psd, int n,
                          fmr_rf_monitor_levels *out, size_t out_size) {
  if (int rc = derive_args("fmr_rf_monitor_derive", recs && out, "recs or out", n)) return rc;
  double m2 = 0.0, m4 = 0.0;
  unsigned long long nf = 0, seg = 0;
  std::vector<unsigned long long> h(kRfmBins, 0ull);
  for (int i = 0; i < n; i++) {
    const fmr_rf_monitor_record &r = recs[i];
    m2 += r.m2; m4 += r.m4; nf += r.n_finite; seg += r.segments;
    if (hist)
      for (int b = 0; b < kRfmBins; b++) h[b] += hist[(size_t)i * kRfmBins + b];
  }
  const std::vector<double> p = mon_pool_psd(recs, psd, n);
  const double M2 = nf ? m2 / (double)nf : 0.0, M4 = nf ? m4 / (double)nf : 0.0;
  const auto db = db10;
  auto pct = [&](unsigned q) -> double {
    if (!hist || nf == 0) return -INFINITY;
    unsigned long long cum = 0;
    for (int b = 0; b < kRfmBins; b++) {
      cum += h[b];
      if (100ull * cum >= (unsigned long long)q * nf) {
        const int u = b + kRfmBinBase;
        return 10.0 * std::log10(std::ldexp(1.0 + (u & 7) / 8.0, (u >> 3) - 127));
      }
    }
    return -INFINITY;      // (a histogram that holds fewer counts than n_finite says)
  };
  const double d = 2.0 * M2 * M2 - M4, Sc = d > 0.0 ? std::sqrt(d) : 0.0, Nn = M2 - Sc;
  const double ref = 4.0 * M2 * M2;
  fmr_rf_monitor_levels full{};
  full.struct_size = (unsigned)sizeof full;
  full.level_dbfs = db(M2);
  full.carrier_dbfs = db(Sc);
  full.noise_dbfs = db(Nn);
  full.cn_db = Sc > 0.0 ? (Nn > 0.0 ? 10.0 * std::log10(Sc / Nn) : INFINITY) : -INFINITY;
  full.am_rms = M2 > 0.0 ? std::sqrt(std::max(M4 / (M2 * M2) - 1.0, 0.0)) / 2.0 : 0.0;
  full.am_audio_db = M2 > 0.0 ? db(mon_band(p, 750.0, 15000.0, false) / ref) : -INFINITY;
  full.am_pilot_db = M2 > 0.0 ? db(mon_band(p, 18250.0, 19750.0, false) / ref) : -INFINITY;
  full.am_floor_dbc_hz = M2 > 0.0 ? db(mon_band(p, 100000.0, 150000.0, true) / ref) : -INFINITY;
  full.p10_dbfs = pct(10); full.p50_dbfs = pct(50); full.p90_dbfs = pct(90);
  full.n_finite = nf;
  full.segments = seg;
  give_sized(out, out_size, full);
  return FMR_OK;
}

int fmr_filter_table(const char *name, const void **data, int *is_double) {
  struct Ent { const char *name; const void *p; int n; int dbl; };
  static const Ent tabs[] = {
      {"jj1bdx_48khz_fmaudio", k_jj1bdx_48khz_fmaudio, 127, 1},
      {"jj1bdx_48khz_nbfmaudio", k_jj1bdx_48khz_nbfmaudio, 63, 1},
      {"jj1bdx_am_48khz_narrow", k_jj1bdx_am_48khz_narrow, 255, 0},
      {"jj1bdx_am_48khz_medium", k_jj1bdx_am_48khz_medium, 255, 0},
      {"jj1bdx_am_48khz_default", k_jj1bdx_am_48khz_default, 255, 0},
      {"jj1bdx_am_48khz_wide", k_jj1bdx_am_48khz_wide, 127, 0},
      {"jj1bdx_nbfm_48khz_default", k_jj1bdx_nbfm_48khz_default, 127, 0},
      {"jj1bdx_nbfm_48khz_narrow", k_jj1bdx_nbfm_48khz_narrow, 127, 0},
      {"jj1bdx_nbfm_48khz_medium", k_jj1bdx_nbfm_48khz_medium, 127, 0},
      {"jj1bdx_nbfm_48khz_wide", k_jj1bdx_nbfm_48khz_wide, 127, 0},
      {"jj1bdx_fm_384kHz_narrow", k_jj1bdx_fm_384kHz_narrow, 127, 0},
      {"jj1bdx_fm_384kHz_medium", k_jj1bdx_fm_384kHz_medium, 127, 0},
      {"jj1bdx_cw_48khz_500hz", k_jj1bdx_cw_48khz_500hz, 2049, 0},
      {"jj1bdx_ssb_48khz_1500hz", k_jj1bdx_ssb_48khz_1500hz, 2049, 0},
      {"ws_usn", ws_taps(), kWsTaps, 1},       // the weak-signal detector's high-pass (built in double at first use)
  };
  if (!name) return FMR_ERR_BAD_ARG;
  for (const auto &e : tabs)
    if (std::strcmp(e.name, name) == 0) {
      if (data) *data = e.p;
      if (is_double) *is_double = e.dbl;
      return e.n;
    }
  return FMR_ERR_BAD_ARG;
}


int fmr_spectrum_create(const fmr_spectrum_config *cfg, size_t cfg_size, fmr_spectrum **out) {
  if (!cfg || !out) { set_err("fmr_spectrum_create: null argument"); return FMR_ERR_BAD_ARG; }
  *out = nullptr;
  fmr_spectrum_config full;
  if (int rc = spec_take_cfg(cfg, cfg_size, full)) return rc;
  fmr_spectrum *s = new fmr_spectrum();
  s->cfg = full;
  if (int rc = s->init()) { delete s; return rc; }
  *out = s;
  return FMR_OK;
}

int fmr_spectrum_create_waterfall(const fmr_spectrum_config *cfg, size_t cfg_size, const fmr_waterfall_config *wf,
                                  size_t wf_size, fmr_spectrum **out) {
  if (!cfg || !wf || !out) { set_err("fmr_spectrum_create_waterfall: null argument"); return FMR_ERR_BAD_ARG; }
  *out = nullptr;
  fmr_spectrum_config full;
  if (int rc = spec_take_cfg(cfg, cfg_size, full)) return rc;
  fmr_waterfall_config w;
  if (int rc = take_sized("fmr_spectrum_create_waterfall", "fmr_waterfall_config", wf, wf_size, w)) return rc;
  if (int rc = wf_check(full, w)) return rc;
  fmr_spectrum *s = new fmr_spectrum();
  s->cfg = full;
  s->wf = w;
  if (int rc = s->init()) { delete s; return rc; }
  *out = s;
  return FMR_OK;
}

void fmr_spectrum_destroy(fmr_spectrum *s) { delete s; }

int fmr_spectrum_process(fmr_spectrum *s, const void *iq, size_t row_stride, size_t n) {
  return spectrum_call(s, iq, row_stride, n, true, 1);
}

int fmr_spectrum_process_device(fmr_spectrum *s, const void *d_iq, size_t row_stride, size_t n, int sync) {
  return spectrum_call(s, d_iq, row_stride, n, false, sync);
}

int fmr_spectrum_synchronize(fmr_spectrum *s) {
  if (!s) return FMR_ERR_BAD_ARG;
  HIPCHK(hipSetDevice(s->cfg.device));
  HIPCHK(hipStreamSynchronize(s->stream));
  return FMR_OK;
}

int fmr_spectrum_read(fmr_spectrum *s, int row, int which, double *out, size_t cap, fmr_spectrum_info *info) {
  if (!s || row < 0 || row >= s->rows || (which != 0 && which != 1)) { set_err("fmr_spectrum_read: bad row or which"); return FMR_ERR_BAD_ARG; }
  const int N = s->N;
  if (cap < (size_t)N) { set_err("fmr_spectrum_read: cap %zu < fft_size %d", cap, N); return FMR_ERR_CAPACITY; }
  if (!out) { set_err("fmr_spectrum_read: out is null"); return FMR_ERR_BAD_ARG; }
  HIPCHK(hipSetDevice(s->cfg.device));
  HIPCHK(hipStreamSynchronize(s->stream));
  unsigned long long cnt[2];
  HIPCHK(hipMemcpy(cnt, s->d_cnt.p + 2 * row, sizeof cnt, hipMemcpyDeviceToHost));
  std::vector<double> v(N, 0.0);
  if (which == 0) {
    HIPCHK(hipMemcpy(v.data(), s->d_sum.p + (size_t)row * N, N * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    std::vector<float> m(N);
    HIPCHK(hipMemcpy(m.data(), s->d_max.p + (size_t)row * N, N * sizeof(float), hipMemcpyDeviceToHost));
    for (int k = 0; k < N; k++) v[k] = m[k];
  }
  const double F = s->cfg.input_rate;
  const double scale = 1.0 / (F * s->sumw2);
  for (int k = 0; k < N; k++) {
    const double x = v[(k + N / 2) & (N - 1)];          // fftshift: element k is bin k - N/2
    out[k] = cnt[0] == 0 ? 0.0 : which == 0 ? x / (double)cnt[0] * scale : x * scale;
  }
  if (info) {
    info->segments = cnt[0];
    info->segments_skipped = cnt[1];
    info->first_segment = s->first_seg;
    info->samples_seen = s->total;
    info->bin_hz = F / N;
    info->enbw_hz = F * s->sumw2 / (s->sumw * s->sumw);
  }
  return N;
}

int fmr_spectrum_read_waterfall(fmr_spectrum *s, int row, float *out, uint32_t *counted, size_t cap_lines,
                                fmr_waterfall_info *info) {
  if (!s || row < 0 || row >= s->rows) { set_err("fmr_spectrum_read_waterfall: bad row"); return FMR_ERR_BAD_ARG; }
  if (s->wf.segments_per_line <= 0) {
    set_err("fmr_spectrum_read_waterfall: the object has no waterfall (it was made by fmr_spectrum_create)");
    return FMR_ERR_BAD_ARG;
  }
  if (cap_lines > 0 && !out) { set_err("fmr_spectrum_read_waterfall: out is null"); return FMR_ERR_BAD_ARG; }
  HIPCHK(hipSetDevice(s->cfg.device));
  HIPCHK(hipStreamSynchronize(s->stream));
  const int N = s->N;
  const unsigned long long R = (unsigned long long)s->wf.segments_per_line, done = s->next_seg / R;
  RecCursor &cur = s->wf_cur;
  cur.catch_up(row, done);
  const unsigned long long first = cur.read[row];
  const double scale = 1.0 / (s->cfg.input_rate * s->sumw2);
  std::vector<unsigned> cnt;
  // the lines are copied straight into `out` and scaled there; cap_lines = 0 reads nothing
  const int n = cur.take(row, done, cap_lines, [&](size_t k0, size_t slot, size_t m) -> int {
    cnt.resize(m);
    HIPCHK(hipMemcpy(out + k0 * N, s->d_wring.p + ((size_t)row * cur.L + slot) * N, m * N * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt.data(), s->d_wring_cnt.p + (size_t)row * cur.L + slot, m * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < m; k++) {
      const double div = s->wf.which == FMR_WATERFALL_MEAN ? (double)cnt[k] : 1.0;
      float *ln = out + (k0 + k) * N;
      for (int i = 0; i < N / 2; i++) {                                // fftshift: element i is bin i - N/2
        const double lo = ln[i], hi = ln[i + N / 2];
        ln[i] = cnt[k] == 0 ? 0.f : (float)(hi / div * scale);
        ln[i + N / 2] = cnt[k] == 0 ? 0.f : (float)(lo / div * scale);
      }
      if (counted) counted[k0 + k] = cnt[k];
    }
    return FMR_OK;
  });
  if (n < 0) return n;
  if (info) {
    info->first_line = first;
    info->lines_ready = done - cur.read[row];
    info->lines_dropped = cur.dropped[row];
    info->line_seconds = (double)R * s->H / s->cfg.input_rate;
  }
  return n;
}

int fmr_spectrum_reset(fmr_spectrum *s) {
  if (!s) return FMR_ERR_BAD_ARG;
  HIPCHK(hipSetDevice(s->cfg.device));
  HIPCHK(hipMemsetAsync(s->d_sum.p, 0, s->d_sum.n * sizeof(double), s->stream));
  HIPCHK(hipMemsetAsync(s->d_max.p, 0, s->d_max.n * sizeof(float), s->stream));
  HIPCHK(hipMemsetAsync(s->d_cnt.p, 0, s->d_cnt.n * sizeof(unsigned long long), s->stream));
  s->first_seg = s->next_seg;
  return FMR_OK;
}

int fmr_find_stations(const double *psd, int fft_size, double input_rate, const fmr_station_rule *rule, fmr_station *out,
                      int cap) {
  if (!psd || !rule || cap < 0 || (cap > 0 && !out)) { set_err("fmr_find_stations: null argument"); return FMR_ERR_BAD_ARG; }
  const int N = fft_size;
  if (N < 2 || (N & (N - 1)) != 0) { set_err("fmr_find_stations: fft_size %d is not a power of two", N); return FMR_ERR_BAD_ARG; }
  if (!(input_rate > 0.0) || !std::isfinite(input_rate)) { set_err("fmr_find_stations: input_rate %g is not > 0", input_rate); return FMR_ERR_BAD_ARG; }
  if (rule->raster_hz <= 0) { set_err("fmr_find_stations: raster_hz %d <= 0", rule->raster_hz); return FMR_ERR_BAD_ARG; }
  if (rule->bandwidth_hz <= 0) { set_err("fmr_find_stations: bandwidth_hz %d <= 0", rule->bandwidth_hz); return FMR_ERR_BAD_ARG; }
  const double p = rule->floor_percentile == 0.0 ? 20.0 : rule->floor_percentile;
  if (!(p >= 0.0 && p < 100.0)) { set_err("fmr_find_stations: floor_percentile %g is outside [0, 100)", p); return FMR_ERR_BAD_ARG; }
  const double F = input_rate, df = F / N;
  const double mab = rule->max_abs_offset_hz != 0 ? (double)rule->max_abs_offset_hz : (F - kFmRate) / 2.0;
  auto fk = [&](int k) { return (double)(k - N / 2) * df; };
  // 1. floor density
  std::vector<double> in_band;
  for (int k = 0; k < N; k++)
    if (std::fabs(fk(k)) <= mab) in_band.push_back(psd[k]);
  if (in_band.empty()) return 0;
  std::sort(in_band.begin(), in_band.end());
  const double floor_d = in_band[(size_t)std::floor(p / 100.0 * (double)(in_band.size() - 1))];
  // 2. candidates, 3. band power
  const double bw = rule->bandwidth_hz, half = bw / 2.0, raster = rule->raster_hz, off = rule->raster_offset_hz;
  struct Cand { double f, B, noise, cen; };
  std::vector<Cand> c;
  for (long long j = (long long)std::ceil((-mab - off) / raster); ; j++) {
    const double f = off + (double)j * raster;
    if (f > mab) break;
    if (std::fabs(f) > mab) continue;
    double B = 0.0, fp = 0.0, pp = 0.0;
    int nb = 0;
    for (int k = 0; k < N; k++)
      if (std::fabs(fk(k) - f) <= half) { B += psd[k] * df; fp += fk(k) * psd[k]; pp += psd[k]; nb++; }
    c.push_back({f, B, floor_d * nb * df, fp / pp});
  }
  // 4. acceptance, 5. output
  int count = 0;
  for (size_t i = 0; i < c.size(); i++) {
    const double snr = spec_db(c[i].B / c[i].noise);
    if (!(snr >= rule->threshold_db)) continue;
    bool keep = true;
    for (size_t q = 0; q < c.size() && keep; q++) {
      const double d = std::fabs(c[q].f - c[i].f);
      if (q == i || !(d > 0.0 && d < bw)) continue;
      if (c[q].B > c[i].B || (c[q].B == c[i].B && c[q].f < c[i].f)) keep = false;
    }
    if (!keep) continue;
    if (count < cap) {
      fmr_station &o = out[count];
      o.offset_hz = (int32_t)c[i].f;
      o.reserved = 0;
      o.level_db = spec_db(c[i].B);
      o.snr_db = snr;
      o.centroid_hz = c[i].cen;
    }
    count++;
  }
  return count;
}

}  // extern "C"
