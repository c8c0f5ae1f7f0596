// chain_shape.hpp -- what a chain IS, decided before anything is built: ChainShape holds everything that follows from
// fmr_config, the environment's switches and the channelizer flag alone, and plan_create() fills it without a single HIP
// call.  It is to fmr_chain::init() what CallPlan / plan_call() are to run(): init() asks for the shape first -- a
// configuration that is refused never opens the device -- and then only builds from it; the call path reads it.
// (Part of fmradion_amd.hip's translation unit, included behind EnvKnobs: it uses that file's constants and set_err.)
#pragma once

struct ChainShape {
  fmr_config cfg{};                    // as handed in, except channel_offset_hz (copied to cb_off: the caller's array need not outlive fmr_create)
  int S = 1, mode = FMR_MODE_FM;
  bool has_rs = false, has_dec = true, fir_enable = false, stereo = false, pilot_shift = false;
  bool enable_mpf = false;
  // Mismatch-based acceptance threshold of the PLL rounds, in units of the convergence scales (phase 1e-7 rad,
  // freq 1e-9, phase error 1e-5, biquad delays 1e-7 relative); env FMR_PLL_RTOL, 0 = off.  The second integration pass of
  // a call in lock sees a boundary mismatch of 8.7 .. 9.0 behind the FAST resampler class and 10.4 behind the R8B class
  // (tools/pll_mismatch.py: 7e4 after the nominal-ramp guess, 0.008 after a third pass): at 16 both are accepted there.
  // Measured against the 0.01 setting (third pass) the audio moves by 1.7e-9 RMS -- a tenth of the float32 front end's
  // own 1.8e-8 deviation from the fp64-accumulating oracle, 6000x inside the 1e-5 target -- and get_pilot_level by
  // up to 2e-6 relative.  (Round 3's 10 put the R8B class one pass -- 0.15 ms per 2^27-sample call -- behind.)
  double pll_rtol = 16.0;
  bool pipelined = false;              // the stages of consecutive calls run beside each other (fmr_chain: "cross-call pipelining")
  double dec_rate = kFmRate;           // the rate the front end delivers: the decoder's, or a front-end-only chain's output_rate
  ResamplerDesign rs, ars;             // IF resampler, FM audio resampler
  // capacities
  size_t max_in = 0, max_mid = 0, max_if = 0, max_amid = 0, max_au = 0;
  int max_blocks = 0;
  int H_in = 0, H_mid = 0, H_if = 0, H_a = 0, H_am = 0, H_pc = 0;
  int ntaps = 0, n_pilotcut = 0, mpf_N = 0, mpf_ref = 0;
  std::vector<float> filter;           // the IF filter's taps (fmr_config.filter_coeff, or AmDecoder's own for the SSB family)
  float h_coeff0 = 0.f;                // filter[0]
  double nbfm_freq_dev = 8000.0;
  bool ssb_like = false;               // SSB / CW / WSPR (AmDecode.cpp:83-90,107-136): mixers before and after the 2049-tap filter
  double af_ref = 0.6, af_rate = 0.001;  // AfSimpleAgc reference / rate (AmDecode.cpp:54-66)
  int in_fmt = 0, in_bps = 8;          // source sample format (fmr_config.input_format) and its bytes per IQ sample
  // ---- front-end kernel forms: plan_create() records what the chain's shape allows, plan_call() picks per call what runs
  enum class StageA : unsigned char { none, pass, bank, fused, decim16, decim2_16, decim2_24, decim };
  enum class StageB : unsigned char { none, fused, poly5h_disc, poly5h, poly4_am, poly4, poly3, poly2, poly_frac, poly };
  // the IF filter: none (FM without it: the block RMS is taken inside the discriminator kernel), the matrix-core form with
  // the discriminator epilogue (FM -f), k_fm_block3 with / without it, the matrix-core form + k_fir_finish (48 kHz modes),
  // k_fm_block2, k_fm_block
  enum class IfForm : unsigned char { none, poly4_disc, block3_disc, block3, poly4_finish, block2, block };
  enum class FusedFe : unsigned char { none, if_only, disc };
  struct FeForms {
    // stage B of a call that takes no upgrade, the first the shape allows of: poly5h (48/125 on the fp16 matrix cores,
    // three-product split), poly4_am (the 3/8 shape of 384 k -> 48 k as sixteen periods per row block: 48/128), poly4 (f32
    // MFMA, 48/125/210), poly3 (Q positions per wave share the LDS reads), poly2, poly_frac (fractional phases), poly
    StageB b = StageB::poly;
    FusedFe fused = FusedFe::none;   // fused front end (kernels_fused.hpp; 10 MS/s class, FM, cf32, no Fs/4): IF samples only, or
                                     // with the discriminator as its epilogue (nothing between resampler and discriminator)
    bool decim16 = false;            // R8B class at 10 MS/s: stage A in the fused front end's matrix-core form (k_ifr_decim16<10, 195>)
    bool poly5h_disc = false;        // R8B class, FM, nothing between resampler and discriminator: the discriminator is k_ifr_poly5h's epilogue
    IfForm fir = IfForm::none;       // the IF filter on the matrix cores: poly4_disc (FM -f, k_ifr_poly4<48, 48, 127, 2, Poly4FirDiscEpi>:
                                     // filter + discriminator + block sums) or poly4_finish (k_ifr_poly4<48, 48, 255 | 127> + k_fir_finish)
  } fe;
  bool poly2_ok = false, poly3_ok = false;   // k_ifr_poly2's / k_ifr_poly3's tables exist (every tiled form reads the first)
  int poly2_tile = 0;                  // staged mid samples per tile, 0 = no tiled stage B
  int poly4_am_tile = 0;
  int poly5h_nkb = 0, poly5h_ea = 0;   // k-blocks of 32 taps; the taps are scaled by 2^ea (the largest into [512, 1024)) ...
  float poly5h_inv_scale = 1.f;        // ... and the results by 2^-ea
  size_t poly5h_lds = 0;
  int qa = 0;                          // stage-A taps per phase of k_ifr_decim2 (16 or 24), 0 = that kernel not applicable
  int hB_pitch = 0;                    // fractional-phase stage B: row pitch of d_hB (floats)
  // channel bank (fmr_config.channel_offset_hz): S channels of one input row, stage A in k_ifr_chan (kernels_chanbank.hpp)
  bool bank = false;
  std::vector<int32_t> cb_off;         // the offsets [Hz]
  unsigned long long cb_F = 0;         // input_rate [Hz]
  // time-parallel recurrences
  int c_pll = 64;                      // PLL chunk length (>= C_PLL_MIN; 32: 0.40 ms, 48: 0.345, 64: 0.33, 96 / 128: 0.47 per 2^27-sample call)
  int H_b = 0;                         // halo of the pre-de-emphasis buffers (>= warm-up)
  size_t max_ck = 0, max_agc_nc = 0, max_dc_nc = 0;
  size_t ck_copy = 0;                  // elements of one copy of d_ck_wraps
  int pll_tick2_per_stream = 0;
  int mask_words = 2;
  static constexpr int kMaxFusedWg = 2048;
  size_t tab_ints = 0;                 // 5*max_blocks block table + 3*max_ck chunk table + (max_blocks+1) first-chunk table + kMaxFusedWg
  // constants of the mode
  PllConst pllc{};
  Iir1Coef deemph{}, am_deemph{};
  BiquadCoef dcblock{}, am_dcblock{};
  DcCoef dk{}, am_dk{};                // the DC block's chunk transitions: FM (chunks of C_DC), AM family (C_AM)
  DeScan de_scan{};                    // pw here; apow points into device memory (the build step sets it)
  float agc_init = 1.f, agc_max = 1e5f, agc_rate = 1e-4f;
  float disc_nf = 1.f, disc_bound = 1.f;
  // MPX-input form (fmr_create_mpx_decoder; kernels_mpxin.hpp): no IF at all -- StageA::none / StageB::none / IfForm::none in
  // every call -- the front end reads mono PCM at 384000 L / M and writes the MPX row; max_in counts frames, max_if MPX samples
  bool mpx_in = false;
  int mi_format = 0, mi_rate = 0, mi_L = 1, mi_M = 1, mi_T = 1, mi_K = 1;
  double mi_gain = 1.0;                // as configured (the default filled in); the kernels take gain M / L
  bool mi_rds = false;
  int in_rows() const { return bank ? 1 : S; }   // rows of the input buffers (d_in, d_in_halo)
};

// ---- DC block: A = [[-a1, -a2], [1, 0]] acts on (w[n-1], w[n-2]); A^chunk by repeated multiplication, then the node
// scan's lane-group transitions (A^(chunk K))^(2^k).  The poles of FM's DC block lie 4.4e-4 from 1 and from each other: A^n has
// entries of n r^n (830 at n = 2048) that cancel on a state whose two words are nearly equal, and a chain of n products in
// double leaves it n^2 2^-53 wrong (4e-10 of A^2048: 130 ulp of the DC block's state in the audio).  So the
// powers are formed in long double (n^2 2^-64) and handed to the kernel as the double next to each entry plus what that
// double leaves (k_dc_nodes: mv2c).
static void mat2_mul(const long double *x, const long double *y, long double *z) {      // z = x y, row-major 2 x 2; z may be x or y
  const long double t[4] = {x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3], x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3]};
  for (int j = 0; j < 4; j++) z[j] = t[j];
}
static DcCoef make_dc_coef(const BiquadCoef &q, int chunk) {
  DcCoef k{q.b0, q.b1, q.b2, q.a1, q.a2, {}, {}, {}, {}};
  const long double a[4] = {-(long double)q.a1, -(long double)q.a2, 1.0L, 0.0L};
  long double ac[4] = {1, 0, 0, 1}, gk[4] = {1, 0, 0, 1};
  auto put = [](const long double *m, double *hi, double *lo) {
    for (int j = 0; j < 4; j++) { hi[j] = (double)m[j]; lo[j] = (double)(m[j] - (long double)hi[j]); }
  };
  for (int i = 0; i < chunk; i++) mat2_mul(a, ac, ac);
  put(ac, k.ac, k.ac_lo);
  for (int i = 0; i < FMR_DC_K; i++) mat2_mul(ac, gk, gk);          // A^(C*K)
  for (int lv = 0; lv < 6; lv++) {
    put(gk, k.agp[lv], k.agp_lo[lv]);
    mat2_mul(gk, gk, gk);
  }
  return k;
}

// A^LPL of the de-emphasis, A = -a1 = exp(-1/tau): the step of the fused de-emphasis scan (DeScan)
static double deemph_step(const Iir1Coef &d) {
  double a = 1.0;
  for (int i = 0; i < FMR_DE_LPL; i++) a *= -d.a1;
  return a;
}

// a stage-A filter as the kernels hold it (rounded to float) is symmetric: the matrix-core forms fold it
static bool taps_symmetric(const ResamplerDesign &rs) {
  for (int k = 0; k < rs.NA / 2; k++)
    if ((float)rs.hA[k] != (float)rs.hA[rs.NA - 1 - k]) return false;
  return true;
}

// ---- stage B, whole-phase form (LT == 0).  Output position q of a period of LB takes tap row phi[q] and starts off[q]
// mid samples into the period's MB.  The tiled kernels stage 64 periods per tile: tl mid samples.
struct StageBLayout {
  std::vector<int> phi, off;
  long long tl = 0;
  int dmax = 0;                        // k_ifr_poly3: the largest window shift among the Q3 positions a wave shares
  static constexpr int Q3 = 4;
  explicit StageBLayout(const ResamplerDesign &rs) : phi((size_t)rs.LB), off((size_t)rs.LB) {
    for (long long q = 0; q < rs.LB; q++) { phi[q] = (int)((q * rs.MB) % rs.LB); off[q] = (int)((q * rs.MB) / rs.LB); }
    tl = 64 * rs.MB + off[rs.LB - 1] + rs.TB;
    for (long long g = 0; g * Q3 < rs.LB; g++)
      dmax = std::max(dmax, off[std::min<long long>(g * Q3 + Q3 - 1, rs.LB - 1)] - off[g * Q3]);
  }
};
// One predicate per form.  poly2: 64 periods fit the LDS a workgroup may ask for.  poly3: also the shift of the positions a
// wave shares fits the rows' zero padding, with 64 samples of slack (the last 8-sample step may run past the union window).
static bool poly2_fits(const ResamplerDesign &rs, const StageBLayout &l) { return l.tl * 8 <= 98304 && rs.LB <= 4096; }
static bool poly3_fits(const ResamplerDesign &rs, const StageBLayout &l) {
  return poly2_fits(rs, l) && l.dmax <= FMR_POLY_PADZ - 8 && (l.tl + 64) * 8 <= 98304;
}
// poly4: 48/125 with 210 taps per phase, the banded f32 matrix-core kernel.  poly4_am: 384 k -> 48 k (config 3) -- sixteen
// periods of 3 outputs / 8 mid samples are one period of 48 / 128, output 3 a + b of it starts 8 a + off[b] samples in and
// takes phase row phi[b] -- so the same kernel serves it (round 6: k_ifr_poly3 took 0.147 ms per 2.1 M IF samples).
// Both share poly3's tile.
static bool poly4_fits(const ResamplerDesign &rs, const StageBLayout &l) {
  return poly3_fits(rs, l) && rs.LB == 48 && rs.MB == 125 && rs.TB == 210;
}
static bool poly4_am_fits(const ResamplerDesign &rs, const StageBLayout &l, const EnvKnobs &env) {
  return poly3_fits(rs, l) && rs.LB == 3 && rs.MB == 8 && rs.TB == 214 && !env.no_fused;
}
// poly5h: any other even stage-B length at 48 / 125 (R8B class: TB = 3122) as a dense product on the fp16 matrix cores, A
// fragments streamed through LDS in chunks of KCH k-blocks of 32 taps.  It reads poly2's tables and no padded rows: it needs
// what poly2 needs, not what poly3 needs.
struct Poly5hGeom { int nkb = 0; size_t lds = 0; };
static bool poly5h_fits(const ResamplerDesign &rs, const StageBLayout &l, Poly5hGeom &g) {
  if (!(poly2_fits(rs, l) && rs.LB == 48 && rs.MB == 125 && rs.TB != 210 && (rs.TB & 1) == 0)) return false;
  constexpr int KCH = FMR_POLY5H_KCH;
  g.nkb = (((l.off[47] + rs.TB + 31) / 32 + KCH - 1) / KCH) * KCH;
  const size_t x_len = (size_t)((((int)l.tl + 64 + 127) / 128) * 128 + 96);
  g.lds = 8 * x_len + 2 * (size_t)KCH * 3 * 2 * 64 * 16;      // (planes + two A chunks; the results are staged over the A buffers)
  return g.lds <= 160 * 1024 - 64 && (size_t)63 * 125 + 32 * (size_t)g.nkb <= x_len && x_len <= 48 * 256;
}

// Stage B of a call that takes no upgrade: the first form, in this order, whose predicate holds; the geometry of a form is
// set where the form is chosen.
static void plan_stage_b(ChainShape &sh, const EnvKnobs &env) {
  using StageB = ChainShape::StageB;
  const ResamplerDesign &rs = sh.rs;
  if (rs.LT) { sh.fe.b = StageB::poly_frac; return; }
  const StageBLayout l(rs);
  sh.poly2_ok = poly2_fits(rs, l); sh.poly3_ok = poly3_fits(rs, l);
  const int tile3 = (int)l.tl + 64;
  Poly5hGeom g5;
  if (poly5h_fits(rs, l, g5)) {
    sh.fe.b = StageB::poly5h; sh.poly2_tile = tile3;
    double tmax = 0.0;
    for (double v : rs.hB) tmax = std::max(tmax, (double)std::fabs((float)v));
    if (tmax > 0.0) { int e2; (void)std::frexp(tmax, &e2); sh.poly5h_ea = 10 - e2; }      // tmax 2^ea in [512, 1024)
    sh.poly5h_nkb = g5.nkb; sh.poly5h_lds = g5.lds; sh.poly5h_inv_scale = std::ldexp(1.0f, -sh.poly5h_ea);
  } else if (poly4_am_fits(rs, l, env)) {
    sh.fe.b = StageB::poly4_am; sh.poly2_tile = tile3;
    sh.poly4_am_tile = 64 * 128 + Poly4Shape<48, 128, 214>::off(47) + rs.TB + 64;
  } else if (poly4_fits(rs, l)) {
    sh.fe.b = StageB::poly4; sh.poly2_tile = tile3;
  } else if (sh.poly3_ok) {
    sh.fe.b = StageB::poly3; sh.poly2_tile = tile3;
  } else if (sh.poly2_ok) {
    sh.fe.b = StageB::poly2; sh.poly2_tile = (int)l.tl;
  } else {
    sh.fe.b = StageB::poly;
  }
}

// ---- channel bank (fmr_config.channel_offset_hz; DESIGN.md "Channel bank") ----
// The rules of a bank.  Stage-A shapes in the kernel's range: D = 2 .. 24 (the LDS span of 64 outputs stays under 60 KB)
// and NA <= 400 (the taps of a group of channels stay in the scalar cache's reach).  A channelizer
// (fmr_create_channelizer) is a bank without a decoder: the same rules, with output_rate as the target rate where a
// decoder bank has its decoder's rate.
constexpr int kBankMaxD = 24, kBankMaxNA = 400;
static int check_bank(const fmr_config *c, bool channelizer) {
  if (channelizer) {
    if (c->mode != FMR_MODE_NONE || !c->enable_resampler) {
      set_err("channelizer: needs a front-end-only chain with the IF resampler (mode = -1, enable_resampler = 1); "
              "a decoder bank is fmr_create with channel_offset_hz");
      return FMR_ERR_UNSUPPORTED;
    }
    if (!c->channel_offset_hz) {
      set_err("channelizer: channel_offset_hz is NULL (it needs n_streams offsets, one per channel)");
      return FMR_ERR_BAD_ARG;
    }
  } else if (c->mode == FMR_MODE_NONE || !c->enable_resampler) {
    set_err("channel bank: needs a decoder chain with the IF resampler (enable_resampler = 1, mode != -1)");
    return FMR_ERR_UNSUPPORTED;
  }
  const char *const who = channelizer ? "channelizer" : "channel bank";
  if (c->input_format != FMR_IQ_CF32) {
    set_err("%s: input_format must be FMR_IQ_CF32 (convert raw samples on the host)", who);
    return FMR_ERR_UNSUPPORTED;
  }
  if (c->enable_fourth_down) {
    set_err("%s: enable_fourth_down must be 0 (add input_rate / 4 to the offsets instead)", who);
    return FMR_ERR_BAD_ARG;
  }
  const double F = c->input_rate;
  if (!(F >= 1.0 && F < 4294967296.0) || F != std::floor(F)) {
    set_err("%s: input_rate %.6f is not a whole number of hertz (ppm-corrected rates are not supported)", who, F);
    return FMR_ERR_UNSUPPORTED;
  }
  // the rate stage B delivers: the decoder's, or a channelizer's output_rate (0: the FM IF rate, as for any front-end-only chain)
  const double dec_rate = channelizer ? (c->output_rate > 0 ? c->output_rate : kFmRate)
                                      : c->mode == FMR_MODE_FM ? kFmRate : kAmRate;
  const char *const rate_name = channelizer ? "output_rate" : "decoder rate";
  for (int s = 0; s < c->n_streams; s++) {
    const double f = (double)c->channel_offset_hz[s];
    if (std::fabs(f) > 0.5 * (F - dec_rate)) {
      set_err("%s: |channel_offset_hz[%d]| = %.0f Hz exceeds (input_rate - %s) / 2 = %.0f Hz", who, s,
              std::fabs(f), rate_name, 0.5 * (F - dec_rate));
      return FMR_ERR_BAD_ARG;
    }
  }
  if (c->resampler_class != FMR_RESAMPLER_FAST && c->resampler_class != FMR_RESAMPLER_R8B) return FMR_OK;   // (plan_front_end refuses it)
  ResamplerDesign d;
  const bool ok = c->resampler_class == FMR_RESAMPLER_R8B ? d.design(F, dec_rate, kR8bAtten, kR8bPassFrac, true)
                                                          : d.design(F, dec_rate, kIfAtten);
  if (!ok) return FMR_OK;     // (plan_front_end refuses the ratio)
  if (d.D < 2 || d.D > kBankMaxD || d.NA > kBankMaxNA) {
    set_err("%s: stage-A shape D = %d, NA = %d (%.0f -> %.0f Hz) is outside the bank kernel's range "
            "(D = 2 .. %d, NA <= %d)", who, d.D, d.D == 1 ? 1 : d.NA, F, dec_rate, kBankMaxD, kBankMaxNA);
    return FMR_ERR_UNSUPPORTED;
  }
  return FMR_OK;
}

// ---- the IF resampler: its design, what it may be refused for, the forms of both stages
static int plan_front_end(ChainShape &sh, const EnvKnobs &env) {
  const fmr_config &c = sh.cfg;
  ResamplerDesign &rs = sh.rs;
  ChainShape::FeForms &fe = sh.fe;
  if (c.resampler_class != FMR_RESAMPLER_FAST && c.resampler_class != FMR_RESAMPLER_R8B) {
    set_err("unknown resampler_class %d", c.resampler_class);
    return FMR_ERR_BAD_ARG;
  }
  const bool r8b = c.resampler_class == FMR_RESAMPLER_R8B;
  if (!(r8b ? rs.design(c.input_rate, sh.dec_rate, kR8bAtten, kR8bPassFrac, true) : rs.design(c.input_rate, sh.dec_rate, kIfAtten))) {
    set_err("resampling ratio %.9g -> %.9g is outside the supported design range", c.input_rate, sh.dec_rate);
    return FMR_ERR_UNSUPPORTED;
  }
  if (rs.D == 1) {  // stage A degenerates to a copy (one unit tap)
    rs.NA = 1; rs.hA.assign(1, 1.0);
  }
  if (sizeof(float2) * ((size_t)64 * rs.D + rs.NA - 1) > 60000) {
    set_err("decimation %d of the front end is outside the supported range", rs.D);
    return FMR_ERR_UNSUPPORTED;
  }
  // the generic stage-B kernels stage a window of (255 MB / LB + TB + 6) mid samples in LDS (64 KB without an attribute)
  const unsigned long long span = (255ull * (unsigned long long)rs.MB) / (unsigned long long)rs.LB + (unsigned long long)rs.TB + 6;
  if (span * sizeof(float2) > 65536) {
    set_err("resampling ratio %.9g -> %.9g: stage B needs %d taps per phase at this ratio and class, more than the kernels stage",
            c.input_rate, sh.dec_rate, rs.TB);
    return FMR_ERR_UNSUPPORTED;
  }
  sh.H_in = rs.NA - 1 + rs.D;
  sh.H_mid = rs.TB;
  sh.max_mid = sh.max_in / rs.D + 2;
  sh.max_if = (size_t)((double)sh.max_in * rs.L / rs.M) + 4;
  if (rs.LT) sh.hB_pitch = (rs.TB + 3) & ~3;      // fractional-phase form: rows padded to a multiple of four taps (float4 row loads)
  if (rs.D >= 2) {       // k_ifr_decim2: q taps per phase, rounded up to 16 or 24
    int q = (rs.NA + rs.D - 1) / rs.D;
    if (q & 1) q++;
    const int qa2 = (q <= 16) ? 16 : 24;     // 24: stage A of the R8B class (195 taps at D = 10), cf32 input only
    const size_t lds2 = sizeof(float2) * ((size_t)rs.D * decim2_pad(qa2) + 2);   // + the spare slot
    if (q <= 24 && (qa2 == 16 || sh.in_fmt == 0) && lds2 <= 64000 && (size_t)rs.D * (kDecim2Out + qa2) <= (size_t)16 * kDecim2Out) sh.qa = qa2;
  }
  if (sh.in_fmt != 0 && sh.qa != 16) {
    // the fused sample conversion lives in the v2 front-end kernel only: refuse the chain now, not on every call
    set_err("input_format != cf32 needs the FAST resampler class and a source rate with integer pre-decimation >= 2 (%.0f -> %.0f Hz gives D = %d): "
            "convert on the host or use cf32 input", c.input_rate, sh.dec_rate, rs.D);
    return FMR_ERR_UNSUPPORTED;
  }
  // what the matrix-core front ends ask of the input: cf32, no Fs/4 shift, not a bank, not switched off
  const bool plain_in = sh.in_fmt == 0 && !c.enable_fourth_down && !sh.bank && !env.no_fused;
  const bool direct_disc = sh.mode == FMR_MODE_FM && !c.fmfilter_enable && c.multipath_stages == 0;   // nothing between resampler and discriminator
  plan_stage_b(sh, env);
  fe.decim16 = rs.D == 10 && rs.NA == 195 && plain_in && !env.serial && taps_symmetric(rs);
  // fused front end: the 10 MS/s shape (D = 10, NA = 103) with a symmetric stage-A filter in front of poly4's stage B, FM.
  // Without IF FIR and equaliser the discriminator reads the IF directly and is the kernel's epilogue; with either of them
  // the epilogue stores the IF samples and the chain goes on as usual.
  fe.fused = !(fe.b == ChainShape::StageB::poly4 && rs.D == kFusedD && rs.NA == kFusedNA && taps_symmetric(rs) && sh.mode == FMR_MODE_FM && plain_in)
                 ? ChainShape::FusedFe::none : direct_disc ? ChainShape::FusedFe::disc : ChainShape::FusedFe::if_only;
  fe.poly5h_disc = fe.b == ChainShape::StageB::poly5h && direct_disc && sh.in_fmt == 0 && !env.no_fused;
  return FMR_OK;
}

// ---- the decoder's constants and the capacities behind the IF, by mode
static int plan_decoder(ChainShape &sh) {
  const fmr_config &c = sh.cfg;
  const int mode = sh.mode;
  if (mode == FMR_MODE_FM) {
    sh.stereo = c.stereo != 0;
    sh.pilot_shift = c.pilot_shift != 0;
    sh.enable_mpf = c.multipath_stages > 0;
    sh.agc_init = 1.0f; sh.agc_max = 100000.0f; sh.agc_rate = 0.0001f;     // FmDecode.cpp:74
    sh.disc_nf = (float)((75000.0 / kFmRate) * 2.0 * M_PI);                 // PhaseDiscriminator.cpp:28
    sh.disc_bound = (float)(1.0 / ((75000.0 / kFmRate) * 2.0));             // :30
    const double freq = 19000.0 / kFmRate, bw = 30 / kFmRate;               // PilotPhaseLock.h:31-35
    PllConst &p = sh.pllc;
    p.minfreq = (freq - bw) * 2.0 * M_PI;
    p.maxfreq = (freq + bw) * 2.0 * M_PI;
    p.bq_b0 = 1.46974784e-06; p.bq_a1 = -1.99682419; p.bq_a2 = 0.996825659;  // PilotPhaseLock.cpp:48
    p.lf_b0 = 0.000304341788; p.lf_b1 = -0.000304324564;                      // :51
    p.lock_delay = int(15.0 / bw);
    p.pilot_frequency = 19000;
    p.minsignal = 0.001;
    const double de = c.deemphasis_us;
    sh.deemph = lowpass_rc((de == 0) ? 1.0 : (de * kFmRate * 1.0e-6));      // FmDecode.cpp:67-70
    sh.dcblock = highpass_iir(0.0001);                                       // FmDecode.cpp:62
    double pwr = deemph_step(sh.deemph);
    for (int j = 0; j < 7; j++) { sh.de_scan.pw[j] = pwr; pwr *= pwr; }
    sh.dk = make_dc_coef(sh.dcblock, C_DC);
    ResamplerDesign &ars = sh.ars;
    if (!ars.design(kFmRate, kPcmRate, kAudioAtten)) { set_err("audio resampler design failed"); return FMR_ERR_UNSUPPORTED; }
    if (ars.D == 1) { ars.NA = 1; ars.hA.assign(1, 1.0); }
    sh.H_a = ars.NA - 1 + ars.D;
    sh.H_am = ars.TB;
    sh.n_pilotcut = 127;                                                     // jj1bdx_48khz_fmaudio, FmDecode.cpp:48-49
    sh.H_pc = sh.n_pilotcut - 1;
    sh.max_amid = sh.max_if / ars.D + 2;
    sh.max_au = (size_t)((double)sh.max_if * ars.L / ars.M) + 4;
    sh.H_b = FMR_DE_WARMUP + sh.H_a;           // warm-up of the fused de-emphasis reaches below the oldest stage-A tap
    sh.ck_copy = (size_t)sh.S * sh.max_ck;
    sh.pll_tick2_per_stream = (int)((sh.max_ck / FMR_NODE_GRP + 2) / FMR_NODE_GRP2 + 2);
    sh.mask_words = (std::max(sh.c_pll, 128) + 63) / 64;   // wrap bit masks: one word per 64 samples of a chunk
    sh.max_dc_nc = sh.max_au / C_DC + 2;
    // MultipathFilter(m_enable ? stages : 1)  (FmDecode.cpp:79)
    const unsigned stages = sh.enable_mpf ? c.multipath_stages : 1;
    sh.mpf_N = (int)(stages * 4 + 1);
    sh.mpf_ref = (int)(stages * 3 + 1);
  } else if (mode == FMR_MODE_NBFM) {
    sh.nbfm_freq_dev = (c.nbfm_freq_dev > 0) ? c.nbfm_freq_dev : 8000.0;    // NbfmDecode.h:39 freq_dev_normal
    sh.agc_init = 1.0f; sh.agc_max = 100000.0f; sh.agc_rate = 0.0001f;      // NbfmDecode.cpp:43
    sh.disc_nf = (float)((sh.nbfm_freq_dev / kAmRate) * 2.0 * M_PI);        // NbfmDecode.cpp:35, PhaseDiscriminator.cpp:28
    sh.disc_bound = (float)(1.0 / ((sh.nbfm_freq_dev / kAmRate) * 2.0));
    sh.n_pilotcut = 63;                                                      // jj1bdx_48khz_nbfmaudio, NbfmDecode.cpp:39
    sh.H_b = sh.n_pilotcut - 1;
    sh.max_au = sh.max_if;
  } else {
    const bool cw_like = (mode == FMR_MODE_CW || mode == FMR_MODE_WSPR);
    sh.agc_init = 1.0f; sh.agc_max = 1000000.0f; sh.agc_rate = cw_like ? 0.0006f : 0.0003f;   // AmDecode.cpp:71-77
    sh.af_ref = sh.ssb_like ? 0.24 : 0.6;                                    // AmDecode.cpp:54-66
    sh.af_rate = cw_like ? 0.00125 : 0.001;
    sh.am_dcblock = highpass_iir(60 / kAmRate);                              // AmDecode.cpp:45
    sh.am_deemph = lowpass_rc(100 * kPcmRate * 1.0e-6);                      // AmDecode.cpp:49
    sh.am_dk = make_dc_coef(sh.am_dcblock, C_AM);
    sh.max_au = sh.max_if;
  }
  return FMR_OK;
}

// ---- MPX input (fmr_create_mpx_decoder): what its two structs may hold, and the geometry of the rate
static inline int mpx_in_taps_per_sample(int L, int M, int T) { return (int)(((long long)T * L + M - 1) / M); }
static int plan_mpx_input(ChainShape &sh, const fmr_mpx_input_config &in) {
  const char *fn = "fmr_create_mpx_decoder";
  const fmr_config &c = sh.cfg;
  if (c.mode != FMR_MODE_FM) {
    set_err("%s: mode %d: the MPX input feeds the FM decoder (mode = FMR_MODE_FM)", fn, c.mode);
    return FMR_ERR_UNSUPPORTED;
  }
  if (c.fmfilter_enable) { set_err("%s: fmfilter_enable: the IF filter works on IF samples, and an MPX input has none", fn); return FMR_ERR_UNSUPPORTED; }
  if (c.multipath_stages > 0) { set_err("%s: multipath_stages %u: the equaliser works on IF samples, and an MPX input has none", fn, c.multipath_stages); return FMR_ERR_UNSUPPORTED; }
  if (c.input_format != FMR_IQ_CF32) { set_err("%s: input_format %d: the PCM format is fmr_mpx_input_config.format; input_format must stay FMR_IQ_CF32 (0)", fn, c.input_format); return FMR_ERR_UNSUPPORTED; }
  if (c.enable_fourth_down) { set_err("%s: enable_fourth_down: there is no IQ input to shift", fn); return FMR_ERR_UNSUPPORTED; }
  if (c.enable_resampler) { set_err("%s: enable_resampler must be 0: the IF resampler works on IQ; the PCM rate is fmr_mpx_input_config.rate", fn); return FMR_ERR_BAD_ARG; }
  if (c.channel_offset_hz) { set_err("%s: channel_offset_hz must be NULL: a channel bank cuts an IQ capture", fn); return FMR_ERR_BAD_ARG; }
  if (in.format != FMR_PCM_S16 && in.format != FMR_PCM_F32) {
    set_err("%s: format %d is neither FMR_PCM_S16 (0) nor FMR_PCM_F32 (1)", fn, in.format);
    return FMR_ERR_BAD_ARG;
  }
  const int rate = in.rate == 0 ? kMpxRateIn : in.rate;
  int L, M, T;
  if (!design_mpx_rate(rate, L, M, T, nullptr)) {
    set_err("%s: rate %d is not 0, 384000 or a whole rate in 96000 .. 384000 with L = rate / gcd(rate, 384000) <= %d", fn, in.rate, kOutRateMaxL);
    return FMR_ERR_BAD_ARG;
  }
  if (c.input_rate != 0.0 && c.input_rate != (double)rate) {
    set_err("%s: input_rate %.9g is neither 0 nor the PCM rate %d", fn, c.input_rate, rate);
    return FMR_ERR_BAD_ARG;
  }
  const double gain = in.gain == 0.0 ? 2.0 : in.gain;
  if (!std::isfinite(gain) || !(gain > 0.0)) { set_err("%s: gain %g is not finite and > 0 (0 = 2.0)", fn, in.gain); return FMR_ERR_BAD_ARG; }
  if (in.rds != 0 && in.rds != 1) { set_err("%s: rds %d is neither 0 nor 1", fn, in.rds); return FMR_ERR_BAD_ARG; }
  sh.mpx_in = true;
  sh.mi_format = in.format; sh.mi_rate = rate; sh.mi_L = L; sh.mi_M = M; sh.mi_T = T;
  sh.mi_K = T > 1 ? mpx_in_taps_per_sample(L, M, T) : 1;
  sh.mi_gain = gain; sh.mi_rds = in.rds != 0;
  sh.cfg.input_rate = (double)rate;
  return FMR_OK;
}

// The whole shape, or the refusal: every rule a configuration can break, in one order, with no device in sight.
// mpx_in != nullptr: the MPX-input form (fmr_create_mpx_decoder).
static int plan_create(ChainShape &sh, const fmr_config *c, const EnvKnobs &env, bool channelizer,
                       const fmr_mpx_input_config *mpx_in = nullptr) {
  sh = ChainShape{};
  sh.cfg = *c;
  if (mpx_in) { if (int rc = plan_mpx_input(sh, *mpx_in)) return rc; }
  const int S = sh.S = c->n_streams, mode = sh.mode = c->mode;
  if (env.x_cpll >= C_PLL_MIN) sh.c_pll = env.x_cpll;
  if (env.pll_rtol >= 0.0) sh.pll_rtol = env.pll_rtol;
  if (S < 1 || c->max_block_len == 0 || c->max_blocks < 1) { set_err("bad capacity / n_streams"); return FMR_ERR_BAD_ARG; }
  if (mode != FMR_MODE_NONE && (mode < FMR_MODE_FM || mode > FMR_MODE_WSPR)) {
    set_err("mode %d is not on the hot path (FM, AM, DSB only)", mode);
    return FMR_ERR_UNSUPPORTED;
  }
  sh.has_dec = (mode != FMR_MODE_NONE);
  // MultipathFilter(stages) holds 4 stages + 1 taps; the equaliser kernel takes up to kMaxMpfTaps of them (k_mpf4<20>)
  if (mode == FMR_MODE_FM && c->multipath_stages > (kMaxMpfTaps - 1) / 4) {
    set_err("multipath_stages %u is above %d: the equaliser holds 4 stages + 1 taps, %d at most", c->multipath_stages,
            (kMaxMpfTaps - 1) / 4, kMaxMpfTaps);
    return FMR_ERR_UNSUPPORTED;
  }
  if (c->channel_offset_hz || channelizer) {
    if (int rc = check_bank(c, channelizer)) return rc;
    sh.bank = true;
    sh.cb_off.assign(c->channel_offset_hz, c->channel_offset_hz + S);
    sh.cb_F = (unsigned long long)c->input_rate;
    sh.cfg.channel_offset_hz = nullptr;
  }
  // The stages of consecutive calls run beside each other for FM chains with the resampler (the default; FMR_PIPELINE=0
  // or fmr_config.in_order: one in-order chain per call)
  sh.pipelined = mode == FMR_MODE_FM && c->enable_resampler != 0 && !env.serial && env.pipeline != 0 && c->in_order == 0;
  sh.dec_rate = (mode == FMR_MODE_FM || mode == FMR_MODE_NONE) ? kFmRate : kAmRate;
  if (mode == FMR_MODE_NONE && c->output_rate > 0) sh.dec_rate = c->output_rate;     // IfResampler(in, out), IfResampler.h:35
  sh.has_rs = c->enable_resampler != 0;
  sh.max_blocks = c->max_blocks;
  sh.max_in = c->max_block_len * (size_t)c->max_blocks;
  sh.max_in = (sh.max_in + 15) & ~(size_t)15;          // row pitch keeps every stream 16-byte aligned in every format
  sh.in_fmt = c->input_format;
  if (sh.in_fmt < 0 || sh.in_fmt > 3) { set_err("input_format %d unknown", sh.in_fmt); return FMR_ERR_BAD_ARG; }
  sh.in_bps = sh.in_fmt == 0 ? 8 : sh.in_fmt == 1 ? 4 : 2;
  if (sh.in_fmt != 0 && !c->enable_resampler) {
    set_err("input_format != cf32 is converted inside the front-end kernel: enable_resampler must be set");
    return FMR_ERR_UNSUPPORTED;
  }
  if (sh.has_rs) {
    if (int rc = plan_front_end(sh, env)) return rc;
  } else if (sh.mpx_in) {
    sh.max_if = (size_t)(((unsigned long long)sh.max_in * (unsigned)sh.mi_M + (unsigned)sh.mi_L - 1) / (unsigned)sh.mi_L) + 4;   // MPX samples: ceil(max_in M / L) + 4
  } else {
    sh.max_if = sh.max_in;
  }
  sh.ntaps = c->n_filter_coeff;
  if (sh.mpx_in) sh.ntaps = 0;         // (nothing of the IF: no filter taps, no IF halo)
  sh.ssb_like = (mode == FMR_MODE_USB || mode == FMR_MODE_LSB || mode == FMR_MODE_CW || mode == FMR_MODE_WSPR);
  const float *filter_src = c->filter_coeff;
  if (sh.ssb_like) {     // AmDecoder's own filters: m_ssbfilter for USB/LSB, m_cwfilter for CW/WSPR (AmDecode.cpp:36,40)
    filter_src = (mode == FMR_MODE_USB || mode == FMR_MODE_LSB) ? k_jj1bdx_ssb_48khz_1500hz : k_jj1bdx_cw_48khz_500hz;
    sh.ntaps = 2049;
  }
  sh.fir_enable = (mode == FMR_MODE_FM) ? (c->fmfilter_enable != 0) : (mode != FMR_MODE_NONE);
  if (sh.has_dec && !sh.mpx_in && (sh.ntaps < 1 || !filter_src)) { set_err("filter_coeff missing"); return FMR_ERR_BAD_ARG; }
  sh.H_if = sh.mpx_in ? 0 : sh.has_dec ? (sh.ntaps > 1 ? sh.ntaps - 1 : 1) : 1;
  sh.max_ck = std::max(sh.max_if / (size_t)sh.c_pll, std::min<size_t>(sh.max_if, (size_t)kSmallCall) / (size_t)kCPllSmall) + (size_t)sh.max_blocks + 2;
  sh.tab_ints = 5 * (size_t)sh.max_blocks + 3 * sh.max_ck + (size_t)sh.max_blocks + 1 + ChainShape::kMaxFusedWg;   // tail: first block of each fused workgroup
  sh.max_agc_nc = sh.max_if / C_AGC + 2;
  if (!sh.has_dec) return FMR_OK;
  if (sh.mpx_in) return plan_decoder(sh);
  sh.filter.assign(filter_src, filter_src + sh.ntaps);
  sh.h_coeff0 = sh.filter[0];
  // the IF filter on the matrix cores (127 or 255 taps): FM -f with the discriminator as the kernel's epilogue, and the
  // 48 kHz modes' filter with k_fir_finish behind it
  const bool mfma_fir = sh.fir_enable && !env.no_fused && !env.serial;
  sh.fe.fir = (mfma_fir && mode == FMR_MODE_FM && sh.ntaps == 127 && c->multipath_stages == 0) ? ChainShape::IfForm::poly4_disc
            : (mfma_fir && mode != FMR_MODE_FM && !sh.ssb_like && (sh.ntaps == 255 || sh.ntaps == 127)) ? ChainShape::IfForm::poly4_finish
            : ChainShape::IfForm::none;
  return plan_decoder(sh);
}
