/*
 * fmradion_amd.h -- C-ABI of the MI355X-native FM/AM demodulation hot path.
 *
 * Drop-in boundary: these entry points are what a
 * binding of the reference's stream loop (main.cpp:879-1002) needs in order
 * to replace
 *     FourthConverterIQ::process   include/FourthConverterIQ.h:38   (main.cpp:916)
 *     IfResampler::process         include/IfResampler.h:35-38      (main.cpp:923)
 *     FmDecoder::process + getters include/FmDecode.h:63-105        (main.cpp:956-957)
 *     AmDecoder::process + getters include/AmDecode.h:48-65         (main.cpp:971-972)
 * Plain pointers and sizes only; no C++ or torch types.  The C++ facade with
 * the reference's class names and signatures is
 * airspy-fmradion_amd/host/fmradion_facade.hpp; the reference-side binding is
 * shown in INTEGRATION.md.
 *
 * One object = one decoder chain for `n_streams` independent IQ streams that
 * all see the same block lengths (batch dimension, config 5 of BASELINE.json).
 * All compute runs in hand-written HIP kernels for gfx950; there is no CPU
 * fallback: every call fails with FMR_ERR_NO_DEVICE when no GPU is present.
 *
 * Error convention: 0 = FMR_OK, negative = error; `*n_out == 0` is the
 * reference's "nothing yet" (empty output vector, FmDecode.cpp:89-92,185-188).
 */
#ifndef FMRADION_AMD_H
#define FMRADION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FMR_OK = 0,
  FMR_ERR_NO_DEVICE = -1,     /* no HIP device / HIP runtime error at create */
  FMR_ERR_BAD_ARG = -2,
  FMR_ERR_UNSUPPORTED = -3,   /* e.g. resampling ratio outside the design range */
  FMR_ERR_CAPACITY = -4,      /* output buffer or configured maximum too small */
  FMR_ERR_HIP = -5            /* HIP runtime failure; see fmr_last_error() */
};

/* ModType values follow include/SoftFM.h:49 */
/* ModType order of the reference (include/SoftFM.h:49) */
enum { FMR_MODE_FM = 0, FMR_MODE_NBFM = 1, FMR_MODE_AM = 2, FMR_MODE_DSB = 3, FMR_MODE_USB = 4, FMR_MODE_LSB = 5,
       FMR_MODE_CW = 6, FMR_MODE_WSPR = 7 };
enum { FMR_IQ_CF32 = 0, FMR_IQ_S16 = 1, FMR_IQ_U8 = 2, FMR_IQ_S8 = 3 };
/* Specification of the IfResampler stand-in ("Resampler specification"; r8brain itself is absent from the
 * reference tree).  FAST: pass band 0.885 x Nyquist, aliases of the pass band rejected by 140 dB, what falls between
 * 0.885 x Nyquist and Nyquist rolls off -- the throughput configuration.  R8B: the defaults of the
 * r8b::CDSPResampler24 the reference constructs (sfmbase/IfResampler.cpp:25-29): pass band 0.98 x Nyquist, stop band
 * from Nyquist on, 180 dB -- the reference-equivalent configuration (a neighbouring station 200 kHz away is filtered
 * exactly as the reference filters it), 15 x the stage-B arithmetic. */
enum { FMR_RESAMPLER_FAST = 0, FMR_RESAMPLER_R8B = 1 };

/* PilotPhaseLock::PpsEvent (include/PilotPhaseLock.h:40-44) + the index of the
 * block (within the call) that produced it. */
typedef struct {
  uint64_t pps_index;
  uint64_t sample_index;
  double block_position;
  uint32_t block;
  uint32_t stream;
} fmr_pps_event;

/* Configuration of one chain.  ZERO-INITIALISE (memset / = {0} / fmr_config cfg{}), then set fields and struct_size:
 * every field added since the first version means "as before" when it is 0, and a field left uninitialised is refused
 * if its value is not one this library knows. */
typedef struct {
  int device;                 /* HIP device ordinal */
  int n_streams;              /* >= 1 independent IQ streams (batch) */
  int mode;                   /* FMR_MODE_FM | _NBFM | _AM | _DSB | _USB | _LSB | _CW | _WSPR (the last four ignore
                               * filter_coeff: AmDecoder uses its built-in 2049-tap SSB / CW tables there) */
  double input_rate;          /* sample rate of the IQ handed to process */
  /* Front end.  0 = the decoder is fed at its own rate (384 kHz FM / 48 kHz
   * AM) and no IfResampler runs (main.cpp:778 enable_downsampling=false). */
  int enable_resampler;
  int enable_fourth_down;     /* FourthConverterIQ(false) before the resampler */
  /* FmDecoder ctor arguments (include/FmDecode.h:63-64) */
  int fmfilter_enable;
  const float *filter_coeff;  /* FM IF filter / AM filter taps (caller-supplied, main.cpp:780-810) */
  int n_filter_coeff;
  int stereo;
  double deemphasis_us;       /* 50 / 75 / 0 */
  int pilot_shift;
  unsigned multipath_stages;
  /* capacity */
  size_t max_block_len;       /* largest input block (samples) per call */
  int max_blocks;             /* largest number of blocks per call */
  /* NbfmDecoder ctor argument (include/NbfmDecode.h:49): full-scale deviation in Hz, 0 = freq_dev_normal (8000) */
  double nbfm_freq_dev;
  /* Source sample format of every `iq` argument (fused ingest: converted while the front-end kernel stages its
   * tile; needs enable_resampler).  Conversions are the reference's: FMR_IQ_U8 = RTL-SDR offset binary
   * (RtlSdrSource.cpp:359-365), the others = what sf_read_float delivers for the FileSource formats
   * S16_LE / S8_LE / U8_LE / FLOAT (FileSource.cpp:120-128,491-531).  `iq` pointers are then pointers to
   * interleaved I,Q samples of that type; counts and strides stay in IQ samples; raw-format device buffers and
   * strides must be 16-byte aligned. */
  int input_format;           /* FMR_IQ_CF32 (default) | FMR_IQ_S16 | FMR_IQ_U8 | FMR_IQ_S8 */
  /* Front-end-only chains (mode = -1): IfResampler(input_rate, output_rate) of include/IfResampler.h:35; 0 = the FM
   * IF rate (384 kHz).  Decoder chains ignore it (their rate is fixed: FmDecode.h:38, AmDecode.h:36). */
  double output_rate;
  int resampler_class;        /* FMR_RESAMPLER_FAST (default) | FMR_RESAMPLER_R8B: specification of the IF resampler */
  /* sizeof(fmr_config) of the header the caller was built against; 0 = not stated (taken as this header's).  The struct
   * grows at its end from version to version: fmr_create refuses a size it does not know instead of reading past a
   * shorter struct or misreading a longer one.  Zero-initialise the whole struct first (an unset field must read 0). */
  unsigned struct_size;
  /* 1: one in-order launch chain per call instead of the pipelined one (front end of call N+1 behind the PLL stage of
   * call N, audio tail a call behind).  For callers that synchronise after every call -- fmr_process / fmr_process_blocks
   * through host buffers, the facade's FmDecoder::process -- the pipelined chain has nothing to overlap and pays for its
   * stage hand-offs: 341 against 303 us per 65536-sample block.  Same audio, bit for bit.  0 (default): pipelined. */
  int in_order;
  /* Channel bank: n_streams frequency offsets in Hz, read and copied at create; NULL (default) = n_streams independent
   * IQ rows as before.  Set, every `iq` argument holds ONE row, the capture (stream_stride is ignored), and stream s
   * decodes  u_s[n] = x[n] exp(-2 pi i ((f_s n) mod F) / F),  F = input_rate,  n = samples since the chain's first
   * sample (across calls of any length): a station at +f_s Hz in the capture's spectrum.  Stage A of the IF resampler
   * runs for all channels in one kernel ("ifr_chan") that reads the capture once per group of channels; everything
   * behind it is the plain chain's with n_streams = the number of channels.  Refused at create ("Channel
   * bank"): front-end-only chains (fmr_create_channelizer builds those) and chains without the resampler, input_format != FMR_IQ_CF32, enable_fourth_down
   * (add F/4 to the offsets instead), an input_rate that is not a whole number of hertz, |f_s| > (input_rate -
   * decoder rate) / 2, and stage-A shapes outside the kernel's range (D = 1, D > 24, NA > 400).  fmr_process takes a
   * bank of one channel only (it returns one audio row).
   * KNOWN LIMITATION: a bank never takes the fused front end, and the stage B it runs instead at some shapes (the banded
   * matrix-core k_ifr_poly4 at 10 MS/s FAST) widens a non-finite input sample to its whole tile of IF samples, where a
   * one-stream chain fed u_s keeps the reference's tap support: around a NaN in the capture a channel's audio can
   * differ from that chain's (the NaN itself never reaches the audio).  In a bank whose blanker acts (fmr_enable_blanker,
   * FMR_NB_ACT) a non-finite capture sample is zeroed before stage A reads it, so nothing is widened.  DESIGN.md,
   * "Channel bank". */
  const int32_t *channel_offset_hz;
} fmr_config;

/* Per-stream status after the most recent call (getters of FmDecode.h:77-105 /
 * AmDecode.h:56-65). */
typedef struct {
  float if_rms;
  float baseband_mean;        /* FM: get_tuning_offset() = baseband_mean * 75000 */
  float baseband_level;
  double pilot_level;         /* = 2 * m_pilot_level */
  int stereo_detected;
  float if_agc_gain;
  double af_agc_gain;         /* AM only */
  double multipath_error;
  double pll_freq_err;
  uint32_t multipath_resets;  /* blocks whose equaliser output was discarded */
  /* time-parallel recurrences of the most recent call: Newton
   * rounds used, and whether the serial fallback kernel had to run */
  int agc_iterations, pll_iterations, agc_fallback, pll_fallback;
  double pll_residual;
  float agc_residual_history[16];   /* residual after each Newton round */
  double pll_residual_history[16];
  double pll_residual_components[8];
  double pll_mismatch_history[16];  /* scaled chunk-boundary mismatch seen by each round's integration pass */
  int pll_mismatch_accepted;        /* 1: the last round was accepted on the mismatch alone (node pass skipped) */
  int af_agc_fallback;              /* AM: 1 = the audio tail (DC block / AfSimpleAgc / de-emphasis) ran in its serial form */
  uint32_t agc_sync_timeouts;       /* FM with the equaliser: times the equaliser kernel gave up waiting for the AGC kernel
                                     * that runs beside it (0 in a healthy chain; every synchronising call that sees a new one
                                     * fails with FMR_ERR_HIP: the audio of that call is void) */
} fmr_status;

typedef struct fmr_chain fmr_chain;

int fmr_create(const fmr_config *cfg, fmr_chain **out);
/* The same for a caller that may have been built against an OLDER header: cfg_size = sizeof(fmr_config) as the caller
 * knows it.  The library reads exactly that many bytes (fields the caller does not have mean "as before") and refuses a
 * size larger than its own.  fmr_create itself can only check the struct_size FIELD, which an older, shorter struct does
 * not contain. */
int fmr_create_sized(const fmr_config *cfg, size_t cfg_size, fmr_chain **out);
/* Channelizer: a channel bank without a decoder -- one capture row in, n_streams rows of IQ out at output_rate.  Row s
 * is IfResampler(input_rate, output_rate) (IfResampler.h:35-38) applied to
 *     u_s[n] = x[n] exp(-2 pi i ((f_s n) mod F) / F),   F = input_rate,  f_s = channel_offset_hz[s],
 * n counted from the chain's first sample: the channel bank's definition with nothing behind the resampler.  cfg_size
 * as for fmr_create_sized (0 = this header's size).  Requires mode = -1, enable_resampler = 1 and channel_offset_hz
 * (n_streams entries, copied); reads input_rate, output_rate (0 = 384 kHz), resampler_class, max_block_len, max_blocks
 * and device.  The bank's rules are checked before the device is opened, with output_rate as the target rate:
 * input_format FMR_IQ_CF32, enable_fourth_down = 0, a whole-hertz input_rate, |f_s| <= (input_rate - output_rate) / 2,
 * stage-A shape D = 2 .. 24 and NA <= 400.  Stage A runs for all channels in "ifr_chan" (fmr_resampler_info 8 reports
 * FMR_CB_MODTAP), stage B in the form a plain chain of the same rate and class takes ("ifr_poly*", mask 7).  Output:
 * fmr_resample_blocks / fmr_resample_blocks_device (fmr_resample for a channelizer of one channel).  A non-finite
 * capture sample widens as in the bank (its KNOWN LIMITATION above): exact in stage A, a whole banded tile of IF
 * samples behind k_ifr_poly4. */
int fmr_create_channelizer(const fmr_config *cfg, size_t cfg_size, fmr_chain **out);
void fmr_destroy(fmr_chain *c);
const char *fmr_last_error(void);
const char *fmr_version(void);

/* Kernel forms of the IF resampler (fmr_resampler_info which = 6 / 7).  The form is picked at create from the design
 * shape, the class, input_format and enable_fourth_down, and again on every call from its size. */
enum {
  FMR_FE_FUSED = 1 << 0,        /* k_ifr_fused: stage A + stage B (+ discriminator) in one kernel (set in both masks) */
  FMR_FE_DECIM16 = 1 << 1,      /* stage A: k_ifr_decim16 (R8B class at 10 MS/s, long calls) */
  FMR_FE_DECIM2_16 = 1 << 2,    /* stage A: k_ifr_decim2, up to 16 taps per phase (also the raw-format ingest) */
  FMR_FE_DECIM2_24 = 1 << 3,    /* stage A: k_ifr_decim2, 17..24 taps per phase (cf32 only) */
  FMR_FE_DECIM = 1 << 4,        /* stage A: k_ifr_decim, the generic form (D = 1, D > 15, long filters) */
  FMR_FE_POLY5H = 1 << 5,       /* stage B: k_ifr_poly5h (48/125, fp16 three-product form) */
  FMR_FE_POLY5H_DISC = 1 << 6,  /* stage B: k_ifr_poly5h with the discriminator epilogue */
  FMR_FE_POLY4 = 1 << 7,        /* stage B: k_ifr_poly4<48, 125, 210> */
  FMR_FE_POLY4_AM = 1 << 8,     /* stage B: k_ifr_poly4<48, 128, 214> (the 3/8/214 shape) */
  FMR_FE_POLY3 = 1 << 9,        /* stage B: k_ifr_poly3 */
  FMR_FE_POLY2 = 1 << 10,       /* stage B: k_ifr_poly2 */
  FMR_FE_POLY_FRAC = 1 << 11,   /* stage B: k_ifr_poly_frac (fractional-phase form) */
  FMR_FE_POLY = 1 << 12         /* stage B: k_ifr_poly, the generic form */
};

/* Kernel forms of a channel bank's stage A (fmr_resampler_info which = 8; fmr_config.channel_offset_hz).  Masks 6 and 7
 * keep their meaning: a bank's stage B is reported in mask 7, and its stage A sets no FMR_FE_* bit. */
enum {
  FMR_CB_MODTAP = 1 << 0        /* k_ifr_chan: modulated complex taps over the shared input tile, one rotation per output */
};

/* Design introspection of the resampler stand-in (DESIGN.md "Resampler
 * specification").  which = 0:D 1:NA 2:LB 3:MB 4:TB 5:LT (rows of the interpolated
 * phase table of the fractional-phase form, 0 = one row per phase); 6 / 7: bitmask of the stage-A / stage-B kernel
 * forms (FMR_FE_*) this chain has launched since create (test introspection); 8: bitmask of the channel-bank kernel
 * forms (FMR_CB_*) launched since create (0 for a chain that is no bank); -1 when no resampler. */
long long fmr_resampler_info(const fmr_chain *c, int which);

/* The product's resampler design on the host (no GPU needed): taps of stage A (stage = 0, NA doubles) or of the
 * polyphase stage B (stage = 1, LB x TB doubles, row = phase; (LT + 1) x TB in the fractional-phase form that ratios
 * with very large LB take, e.g. ppm-corrected source rates, main.cpp:708-711) for in_rate -> out_rate at atten_db;
 * info[0..5] receive D, NA, LB, MB, TB, LT.  Rates that are not whole hertz are taken to the millihertz.  Returns the number of taps of the stage, or a negative error (cap too small / unsupported
 * ratio).  Lets tests check the design against an independent construction without a device. */
long long fmr_design_taps(double in_rate, double out_rate, double atten_db, int stage, double *taps, long long cap,
                          long long *info);
/* The same for a resampler class (FMR_RESAMPLER_FAST / _R8B) of the IF resampler: IfResampler(in_rate, out_rate) as
 * fmr_create builds it (sfmbase/IfResampler.cpp:25-29). */
long long fmr_design_taps_class(double in_rate, double out_rate, int resampler_class, int stage, double *taps,
                                long long cap, long long *info);

/* --- live sources: page-locked host memory for the ring between a driver's callback thread and the decoder thread.
 * Replaces the heap vectors that AirspySource::callback (sfmbase/AirspySource.cpp:488-500) and RtlSdrSource::get_samples
 * (sfmbase/RtlSdrSource.cpp:359-365) fill and DataBuffer (include/DataBuffer.h:35-90) queues: the callback copies the
 * driver's RAW buffer (float pairs, or offset-binary bytes -- fmr_config.input_format converts on the GPU) into a block
 * of the ring, and fmr_process_blocks reads the block in place -- from page-locked memory the host-to-device copy is a
 * DMA at the link rate, without the runtime's pageable staging.  host/fmradion_ring.hpp holds the ring itself.
 * Returns NULL (fmr_last_error() says why) without a HIP device: there is no fallback to pageable memory. */
void *fmr_host_alloc(size_t bytes);
void fmr_host_free(void *p);

/* --- single block, host buffers: the shape of FmDecoder::process(IQSampleVector,
 * SampleVector&) (FmDecode.h:74) for stream 0 of a 1-stream chain.
 * iq: n interleaved complex float samples.  audio: doubles (interleaved L/R when
 * stereo).  */
int fmr_process(fmr_chain *c, const float *iq, size_t n, double *audio,
                size_t audio_cap, size_t *n_audio);

/* --- batched blocks, host buffers.  iq holds n_streams rows of `stream_stride`
 * complex samples; block_len[0..n_blocks) are consecutive block lengths inside
 * each row.  audio holds n_streams rows of audio_stride doubles;
 * audio_len[b] receives the number of doubles block b produced (same for all
 * streams).  Semantics = n_blocks sequential process() calls per stream. */
int fmr_process_blocks(fmr_chain *c, const float *iq, size_t stream_stride,
                       const uint32_t *block_len, int n_blocks, double *audio,
                       size_t audio_stride, uint32_t *audio_len);

/* --- same with device-resident buffers (HBM in, HBM out).
 * sync != 0: returns with the audio of this call in d_audio.
 * sync == 0: returns as soon as the call is enqueued.  THE AUDIO OF AN ASYNCHRONOUS CALL IS COMPLETE ONLY AFTER
 * fmr_synchronize() (or a later call with sync != 0, or any getter: they synchronise).  In the pipelined chain (FM with
 * the resampler, fmr_config.in_order == 0) the audio tail of call N is enqueued together with call N + 1 -- or by
 * fmr_synchronize() -- on a stream of the chain's own: waiting on the device or on a stream of yours
 * (hipDeviceSynchronize, a HIP event, torch.cuda.synchronize) does NOT make the last call's audio complete, because its
 * tail may not have been launched yet.  d_iq, d_audio and audio_len must stay valid until that synchronisation; a chain
 * destroyed before it drops the pending tail (nothing is written into d_audio after fmr_destroy returns).
 * Set fmr_config.in_order = 1 for a chain whose every call is complete on the chain's stream order. */
int fmr_process_blocks_device(fmr_chain *c, const float *d_iq,
                              size_t stream_stride, const uint32_t *block_len,
                              int n_blocks, double *d_audio, size_t audio_stride,
                              uint32_t *audio_len, int sync);
int fmr_synchronize(fmr_chain *c);

/* --- front end only: IfResampler::process (IfResampler.h:35-38).  Valid on a
 * chain created with enable_resampler; bypasses the decoder.  Host buffers.  Stream 0 only; a channelizer of more
 * than one channel is refused (FMR_ERR_BAD_ARG): use fmr_resample_blocks. */
int fmr_resample(fmr_chain *c, const float *iq, size_t n, float *out_iq,
                 size_t out_cap, size_t *n_out);

/* --- front end only, batched: IfResampler::process (IfResampler.h:35-38) for every row and block, host buffers.  Valid
 * on any front-end-only chain with the resampler (mode = -1, enable_resampler): a plain chain reads n_streams input rows
 * of stream_stride samples; a channelizer (fmr_create_channelizer) reads ONE row, the capture (stream_stride is ignored).
 * out_iq holds n_streams rows of out_stride complex samples (interleaved float pairs); out_len[b] receives the number of
 * complex samples block b produced, the same in every row.  Semantics = n_blocks successive fmr_resample calls per row.
 * The output capacity is checked before any state advances: FMR_ERR_CAPACITY leaves the chain as it was, and the call
 * can be retried with more room. */
int fmr_resample_blocks(fmr_chain *c, const float *iq, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                        float *out_iq, size_t out_stride, uint32_t *out_len);
/* The same on device buffers (HBM in, HBM out), with fmr_process_blocks_device's asynchronous contract: the rows are
 * complete after fmr_synchronize() or a later call with sync != 0; out_len is filled before the call returns.  Stage B
 * writes every row straight into d_out_iq (columns [0, out_len sum) of each row, nothing else). */
int fmr_resample_blocks_device(fmr_chain *c, const float *d_iq, size_t stream_stride, const uint32_t *block_len,
                               int n_blocks, float *d_out_iq, size_t out_stride, uint32_t *out_len, int sync);

/* --- FourthConverterIQ::process (include/FourthConverterIQ.h:38-82) on host buffers: multiply by the Fs/4 table,
 * `up` selects FourthConverterIQ(true); `index` (in/out, 0..3) is the object's m_index.  Exact (+-1, +-j swaps).
 * Decoder chains fuse the shift into their front-end kernel instead (enable_fourth_down). */
int fmr_fourth_convert(fmr_chain *c, const float *iq, size_t n, float *out_iq, int up, unsigned *index);

int fmr_get_status(fmr_chain *c, int stream, fmr_status *st);
/* ... for a caller built against an older header: st_size = sizeof(fmr_status) as the caller knows it; the library never
 * writes past it (fmr_status grows at its end). */
int fmr_get_status_sized(fmr_chain *c, int stream, void *st, size_t st_size);
/* PPS events of the most recent call (FmDecode.h:92); returns the count. */
int fmr_get_pps_events(fmr_chain *c, int stream, fmr_pps_event *ev, int cap);
/* get_multipath_coefficients (FmDecode.h:103): interleaved re,im; returns order */
int fmr_get_multipath_coefficients(fmr_chain *c, int stream, float *coeff, int cap);

/* Debug taps for stage-level parity tests: copies an intermediate vector of the
 * most recent call to the host.  which: 0 = IF samples entering the decoder
 * (complex float, 2 floats each), 1 = discriminator output (float),
 * 2 = stereo difference after demod+de-emphasis (double), 3 = mono after
 * de-emphasis (double), 4 = AGC gain sequence (float), 5 = on a chain made by fmr_create_rds, the signed symbol
 * reliabilities rho_k (float) of the symbols the most recent call decided, in symbol order (FMR_ERR_BAD_ARG on a
 * chain without RDS).  Returns element count, or FMR_ERR_BAD_ARG for a
 * tap the most recent call did not leave in memory: behind the fused front end's discriminator epilogue (FM at
 * 10 MS/s without IF filter / equaliser) taps 0, 1 and 4 exist only in a chain created with FMR_DEBUG_TAPS=1 in the
 * environment -- the product keeps those signals on chip.  6 = on a chain whose blanker acts (fmr_enable_blanker,
 * FMR_NB_ACT), the input row `stream` as the front end read it in the most recent call (complex float; `stream` is an
 * input row: 0 for a bank; returns the samples of that call); FMR_ERR_BAD_ARG on every other chain.  7 = on a chain
 * whose IQ corrector acts (fmr_enable_iq_correction, FMR_IQC_ACT), the input row `stream` as the corrector wrote it in the
 * most recent call, ahead of the blanker (complex float, as tap 6); FMR_ERR_BAD_ARG on every other chain. */
long long fmr_debug_read(fmr_chain *c, int stream, int which, void *out, size_t cap_bytes);

/* What this library holds of the HIP runtime right now, in the whole process: device buffers, page-locked host blocks,
 * events and streams, one count each.  0 once every chain and spectrum has been destroyed; a failed create or enable
 * leaves it where it was (tests/test_gpu_lifecycle.py). */
long long fmr_debug_live_resources(void);

/* What fmr_create (channelizer = 0) or fmr_create_channelizer (1) would decide about cfg before it builds anything: the
 * shape step of a create, run by itself.  It opens no device and allocates nothing, so it works on a machine without a
 * GPU.  Returns the create's code and leaves its message in fmr_last_error() when the configuration is refused; FMR_OK
 * fills out.  cfg_size: the size of fmr_config as the caller knows it, 0 = as this library does; out_size likewise. */
typedef struct fmr_chain_shape_info {
  unsigned struct_size;       /* set by the library */
  int D, NA;                  /* the IF resampler's design, as fmr_design_taps_class reports it (all 0 without the resampler) */
  long long LB, MB;
  int TB, LT;
  unsigned stage_b;           /* FMR_FE_* bit of stage B of a call that takes no upgrade (0 without the resampler) */
  int fused;                  /* fused front end: 0 no, 1 IF samples only, 2 with the discriminator as its epilogue */
  int decim16, poly5h_disc;   /* the upgrades of stage A (R8B class) and of poly5h the shape allows */
  int fir;                    /* IF filter on the matrix cores: 0 no, 1 with the discriminator epilogue (FM), 2 + k_fir_finish */
  int qa;                     /* taps per phase of k_ifr_decim2: 16, 24, or 0 (the generic stage A) */
  int pipelined;              /* the stages of consecutive calls run beside each other */
  unsigned long long max_if, max_au;   /* capacity per stream and call: IF samples, audio samples per channel */
  int mpx_in;                 /* 1: the MPX-input form (fmr_debug_mpx_chain_shape): no IF, the front end reads PCM; max_if counts MPX samples */
  int mpx_format, mpx_L, mpx_M, mpx_T, mpx_K;   /* ... its PCM format and geometry (all 0 otherwise) */
} fmr_chain_shape_info;
int fmr_debug_chain_shape(const fmr_config *cfg, size_t cfg_size, int channelizer, fmr_chain_shape_info *out, size_t out_size);

/* Kernel timing with HIP events on the chain's own streams.  enable = 1: every kernel of
 * the most recent call (diagnostics; the extra events cost host time).  enable = 2: only the
 * kernels of the FIR + discriminator stage ("ifr_fused", or "ifr_decim" / "ifr_poly" / "disc", a channel bank's stage A
 * "ifr_chan", and the IF FIR "fm_block" of an FM chain), one entry per launch accumulated until queried
 * (what bench.py uses inside its timed region); enable = 4: the same on every fourth call only (the two event
 * markers of a stage kernel cost 7-10 us on the decoder stream: bench.py samples); enable = 5: as 4, and the fused front
 * end ("ifr_fused") on EVERY call.  The fused front end is timed with the start / stop events of its own dispatch
 * (hipExtLaunchKernelGGL: the command processor's time stamps of the kernel's begin and end, what rocprofv3's kernel
 * trace reads; no marker packets on the stream), the other kernels between two event markers on their stream.
 * Fills names/ms for up to cap entries, returns the count. */
int fmr_get_kernel_times(fmr_chain *c, const char **names, float *ms, int cap);
void fmr_enable_kernel_timing(fmr_chain *c, int enable);

/* enable = 3: trace.  Every instrumented kernel of every call since the mode was switched on keeps its event pair; this
 * call synchronises, fills name / stream (0 decoder, 1 side, 2 AGC [in-order chain], 4 audio tail) / start / end (ms since the
 * first traced launch) for up to cap entries, clears the trace and returns the count.  The schedule of the chain's streams
 * as the GPU ran it, without a profiler in the host's launch path (tools/step_timeline.py). */
int fmr_get_kernel_trace(fmr_chain *c, const char **names, int *streams, float *start_ms, float *end_ms, int cap);

/* Measurement aid (no counterpart in the reference): the rate at which a plain streaming-read kernel (16-byte loads,
 * every CU busy, nothing else) reads `bytes` of device memory at d_buf on this device, best of `reps` passes, in GB/s.
 * bench.py reports it next to the roofline fraction: the 8 TB/s of the roofline is the data-sheet peak, this is what
 * the box the run landed on delivers to a kernel that does nothing but read. */
int fmr_probe_read_bandwidth(int device, const void *d_buf, size_t bytes, int reps, double *gbytes_per_s);

/* Measurement aid (no counterpart in the reference): the shader clock of `device` right now, in MHz -- one wave counts
 * its compute unit's cycle counter over 20 us of the constant 100 MHz clock.  The clock ramps over tens of milliseconds
 * of load after an idle gap and the recurrence kernels of the decoder follow it: bench.py reports it on either side of
 * its timed region (what a 20-step region measures against a stream that runs continuously). */
int fmr_probe_shader_clock(int device, double *mhz);

/* Filter tables of FilterParameters (include/FilterParameters.h:31-49), by name
 * e.g. "jj1bdx_fm_384kHz_medium"; returns the length, *is_double tells the type. */
int fmr_filter_table(const char *name, const void **data, int *is_double);

/* --- RDS (no counterpart in the reference).  An FM chain created with fmr_create_rds decodes the
 * RDS data on the 57 kHz subcarrier of every stream's MPX (every channel of a bank): a device stage behind the
 * discriminator estimates symbol timing and carrier phase from the RDS signal itself (no pilot needed; in phase or in
 * quadrature with 3 x pilot) and hands the bits to a host decoder per stream (airspy-fmradion_amd/host/fmradion_rds.hpp:
 * 26-bit blocks, checkword of g(x) = x^10+x^8+x^7+x^5+x^4+x^3+1 plus the offset words A 0x0FC, B 0x198, C 0x168,
 * C' 0x350, D 0x1B4, acquisition on two consecutive valid syndromes, loss of synchronisation after 8 bad blocks in a row,
 * error correction by burst trapping or soft-decision block repair on request: fmr_set_rds_correction).  The decoded groups do not depend on how the input is cut into blocks and calls.
 * One RDS group: four 16-bit blocks in the order A, B, C (or C'), D, a status per block and the absolute 384 kHz MPX
 * sample index (counted from the chain's first sample) at which the group's first bit starts. */
enum {
  FMR_RDS_OK = 0,             /* the block's syndrome is its position's offset */
  FMR_RDS_CORRECTED = 1,      /* the block was bad and fmr_set_rds_correction's mode repaired it: the 16 bits are the repaired ones */
  FMR_RDS_BAD = 2,            /* syndrome mismatch: the block's 16 bits are as received */
  FMR_RDS_CPRIME = 4          /* block 3 carried offset C' (version-B groups) instead of C */
};
typedef struct {
  uint64_t sample_index;
  uint16_t block[4];
  uint8_t status[4];          /* FMR_RDS_OK | FMR_RDS_CORRECTED | FMR_RDS_BAD, | FMR_RDS_CPRIME on block 3 */
  uint32_t reserved;
} fmr_rds_group;
typedef struct {
  int synced;                 /* 1: block-synchronised after the last bit decoded */
  int reserved;
  uint64_t blocks_ok, blocks_corrected, blocks_bad;
  uint64_t groups_decoded;    /* groups assembled in synchronisation since create */
  uint64_t groups_dropped;    /* ... lost because the stream's queue (256 groups) was full: drain it with fmr_get_rds_groups */
  double injection;           /* estimated amplitude of the RDS subcarrier in MPX units (1.0 = 75 kHz deviation) */
  double timing;              /* symbol timing: where a symbol starts within its period [symbols, 0 .. 1) */
  double carrier_phase;       /* carrier phase estimate [rad] (modulo pi: BPSK) */
  double carrier_offset_hz;   /* tracked offset of the subcarrier from 57 kHz [Hz] */
} fmr_rds_status;

/* fmr_create with the RDS decoder on (cfg_size as for fmr_create_sized, 0 = this header's size).  FMR_MODE_FM chains of
 * every shape fmr_create accepts: with or without the resampler (either class), stereo or mono, -f, the equaliser,
 * ppm-corrected rates, pipelined or in_order, channel banks (a decoder per channel).  Any other mode and front-end-only
 * chains (mode = -1, the channelizer's shape) are refused with FMR_ERR_UNSUPPORTED before the device is opened.  The
 * audio and fmr_status are those of the same chain made by fmr_create: the stage only reads the MPX. */
int fmr_create_rds(const fmr_config *cfg, size_t cfg_size, fmr_chain **out);
/* Drain up to cap groups (oldest first) from stream `stream`'s queue; returns the count.  cap = 0: the number queued.
 * Synchronises like the other getters: after it, the groups of every call issued so far are in the queue (on the
 * asynchronous device path they are complete, like the audio, after fmr_synchronize).  FMR_ERR_BAD_ARG on a chain
 * created without RDS. */
int fmr_get_rds_groups(fmr_chain *c, int stream, fmr_rds_group *groups, int cap);
/* Counters and estimates of stream `stream` (synchronises); st_size = sizeof(fmr_rds_status) as the caller knows it. */
int fmr_get_rds_status(fmr_chain *c, int stream, fmr_rds_status *st, size_t st_size);

/* Error correction of synchronised blocks ("Error correction"; the rules are written out in
 * host/fmradion_rds.hpp).  BURST: the error syndrome of a bad block is looked up among all bursts of up to max_burst
 * bits (1 .. 5; 0 = the default, 2: one wrong symbol is two adjacent wrong bits).  SOFT: the device stage hands over the
 * reliability of every symbol; the soft_symbols (1 .. 8; 0 = 4) least reliable of the block's 27 symbols are flipped in
 * every combination and the cheapest one that gives the expected syndrome is taken if its summed reliability is at most
 * soft_max_cost (>= 0, in units of the symbol level; 0 = 1.0).  Acquisition always works on uncorrected syndromes, and
 * a corrected block neither extends nor ends the run of eight bad blocks that drops the synchronisation. */
enum { FMR_RDS_FEC_OFF = 0, FMR_RDS_FEC_BURST = 1, FMR_RDS_FEC_SOFT = 2 };
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_rds_fec) as the caller knows it (0: fec_size) */
  int mode;                   /* FMR_RDS_FEC_* */
  int max_burst;
  int soft_symbols;
  double soft_max_cost;
} fmr_rds_fec;
/* Synchronises, then sets the correction of every stream / channel of the chain; each decoder takes it from its next
 * block boundary on.  May be called at any time; after fmr_create_rds the mode is OFF, and groups, statuses and audio
 * are then what they were before this call existed.  FMR_ERR_BAD_ARG (fmr_last_error names the field) for an unknown
 * mode, a value out of range, a size larger than this library's fmr_rds_fec, and for a chain created without RDS; the
 * fields are checked before the chain is looked at. */
int fmr_set_rds_correction(fmr_chain *c, const fmr_rds_fec *fec, size_t fec_size);

/* --- Band spectrum and station finder (no counterpart in the reference).  A handle of its own:
 * a Welch power spectrum (mean and peak hold) of n_rows IQ rows on the GPU, and a host-side finder that turns a spectrum
 * into offsets fmr_config.channel_offset_hz takes as they are.
 * Segment j of a row covers the absolute samples [j H, j H + N) (counted from the object's first sample, across calls of
 * any length) and is processed in the call that delivers its last sample; the row's last N samples stay on the device.
 * Periodic windows, built in double and rounded once to fp32: Hann w[n] = 0.5 - 0.5 cos(2 pi n / N); rect w[n] = 1;
 * 4-term Blackman-Harris a = 0.35875, 0.48829, 0.14128, 0.01168.
 * Output (doubles, fftshift order: element k is the bin at (k - N/2) F / N Hz, F = input_rate), density-scaled:
 *     |sum_n w[n] x_j[n] exp(-2 pi i k n / N)|^2 / (F sum w^2)
 * which = 0: the mean over the counted segments, which = 1: their peak hold.  sum psd F / N is the mean power.
 * A segment that holds a non-finite sample is left out of both and counted in segments_skipped.
 * Reproducibility: the per-segment arithmetic does not depend on where a segment falls in a call (the peak hold is
 * bit-identical for any cut of the input into calls); float sums run in a fixed order without atomics (the same cut
 * gives the same bits); the mean's partial sums are fp64 (across cuts it differs only at their rounding). */
enum { FMR_WINDOW_HANN = 0, FMR_WINDOW_RECT = 1, FMR_WINDOW_BLACKMAN_HARRIS = 2 };
typedef struct {
  unsigned struct_size;   /* as fmr_config: 0 = this header's size; a larger size is refused */
  int device;
  int n_rows;             /* 1 .. 65535 independent IQ rows (a plain capture, or a channelizer's K output rows) */
  double input_rate;      /* Hz, > 0 */
  int input_format;       /* FMR_IQ_CF32 | _S16 | _U8 | _S8, converted as fmr_config.input_format */
  int fft_size;           /* N: power of two, 256 .. 16384 */
  int hop;                /* H: 1 .. N; 0 = N / 2 */
  int window;             /* FMR_WINDOW_* */
  size_t max_call_len;    /* largest n per call and row: 1 .. 2^30 */
} fmr_spectrum_config;
typedef struct {
  uint64_t segments;          /* averaged since create / the last reset */
  uint64_t segments_skipped;  /* held a non-finite sample: left out of both the mean and the peak hold */
  uint64_t first_segment;     /* absolute index of the first segment processed since create / the last reset */
  uint64_t samples_seen;      /* per row, since create */
  double bin_hz;              /* input_rate / N */
  double enbw_hz;             /* input_rate * sum w^2 / (sum w)^2 */
} fmr_spectrum_info;
/* Station finder rule (fmr_find_stations): candidates f_c = raster_offset_hz + j raster_hz, |f_c| <= max_abs_offset_hz
 * (0 = (input_rate - 384000) / 2, the channel bank's limit); band = the bins within bandwidth_hz / 2 of f_c; floor =
 * the floor_percentile (0 = 20) percentile of the bins within max_abs (sorted value at floor(p / 100 (M - 1))). */
typedef struct {
  int32_t raster_hz, raster_offset_hz, bandwidth_hz, max_abs_offset_hz;
  double threshold_db, floor_percentile;
} fmr_station_rule;
typedef struct {
  int32_t offset_hz, reserved;
  double level_db;      /* band power, dB re a full-scale complex sinusoid (power 1) */
  double snr_db;        /* band power over floor density x band width */
  double centroid_hz;   /* power-weighted mean frequency of the band */
} fmr_station;
typedef struct fmr_spectrum fmr_spectrum;

/* cfg_size = sizeof(fmr_spectrum_config) as the caller knows it (0 = this header's).  FMR_ERR_BAD_ARG (before the device
 * is opened; fmr_last_error names the field) for an N that is not a power of two in 256 .. 16384, a hop outside 0 .. N,
 * an unknown window or input_format, input_rate <= 0, n_rows outside 1 .. 65535, max_call_len outside 1 .. 2^30 or a size
 * larger than this header's;
 * FMR_ERR_NO_DEVICE for a valid configuration without a device. */
int fmr_spectrum_create(const fmr_spectrum_config *cfg, size_t cfg_size, fmr_spectrum **out);
void fmr_spectrum_destroy(fmr_spectrum *s);
/* n samples of every row: row r at iq + r row_stride IQ samples (row_stride 0 = n), host buffers.  n > max_call_len is
 * refused with FMR_ERR_CAPACITY and leaves the object as it was. */
int fmr_spectrum_process(fmr_spectrum *s, const void *iq, size_t row_stride, size_t n);
/* The same on device buffers with fmr_process_blocks_device's asynchronous contract (sync = 0: d_iq stays valid until
 * fmr_spectrum_synchronize, a call with sync != 0 or fmr_spectrum_read).  Raw-format rows are 16-byte aligned. */
int fmr_spectrum_process_device(fmr_spectrum *s, const void *d_iq, size_t row_stride, size_t n, int sync);
int fmr_spectrum_synchronize(fmr_spectrum *s);
/* Synchronises; writes N doubles of row `row` (which 0 = mean PSD, 1 = peak hold; zeros before any segment was counted)
 * and, if info is not NULL, the row's counters.  Returns N, or FMR_ERR_CAPACITY when cap < N. */
int fmr_spectrum_read(fmr_spectrum *s, int row, int which, double *out, size_t cap, fmr_spectrum_info *info);
/* Zeroes both accumulators and the counts of every row; the segment grid keeps its absolute positions.  A waterfall
 * (below) is left alone: it is a stream that reading drains, its unread lines and its line grid stay as they were. */
int fmr_spectrum_reset(fmr_spectrum *s);

/* --- Waterfall: time-resolved lines of the same spectrum, kept in the same pass over the input.
 * R = segments_per_line, L = max_lines (the ring's depth per row).  Line l of a row is made of the segments j in
 * [l R, (l + 1) R) of that row (absolute indices on the object's segment grid); it is complete in the call that delivers
 * the last sample of segment (l + 1) R - 1 and covers the absolute samples [l R H, ((l + 1) R - 1) H + N).  A segment
 * that holds a non-finite sample is skipped as it is for the accumulators; c_l is the number of counted segments.
 *   FMR_WATERFALL_MEAN: (sum P_j[k]) / c_l over the counted segments, the sum in fp32;
 *   FMR_WATERFALL_PEAK: max P_j[k] over the counted segments;      c_l = 0: all zeros (the count tells).
 * Output: floats in fftshift order, density-scaled by the 1 / (F sum w^2) of fmr_spectrum_read; division and scaling
 * are done in double on the host when the line is read, then rounded once to float.
 * Cut independence: a line's values are bit-identical for any cut of the input into calls, on the host and the device
 * path, whatever else a call holds.  The fp32 additions of a MEAN line run in an order that depends on a segment's index
 * q within its line only: aligned sub-blocks of 8 segments (q / 8; the last one shorter when 8 does not divide R) are
 * each summed one segment after the other, and the sub-block sums are added in sub-block order.  A line a call leaves
 * open carries its state on the device to the next call.
 * Ring overrun: when a row holds L unread lines and another completes, the oldest unread one is overwritten and counted
 * in lines_dropped; processing never fails because of it.  fmr_spectrum_reset leaves the waterfall alone.
 * fmr_spectrum_config and fmr_spectrum_create are unchanged: an object made by fmr_spectrum_create has no waterfall. */
enum { FMR_WATERFALL_MEAN = 0, FMR_WATERFALL_PEAK = 1 };
typedef struct {
  unsigned struct_size;    /* 0 = this header's size; a larger size is refused */
  int segments_per_line;   /* R: 1 .. 65536 */
  int max_lines;           /* L >= 1; n_rows x L x N x 4 bytes <= 1 GiB */
  int which;               /* FMR_WATERFALL_* */
} fmr_waterfall_config;
typedef struct {
  uint64_t first_line;     /* absolute index of the first line returned */
  uint64_t lines_ready;    /* complete lines still unread after this call */
  uint64_t lines_dropped;  /* since create: overwritten unread (of this row) */
  double line_seconds;     /* R * H / input_rate */
} fmr_waterfall_info;
/* Checks cfg exactly as fmr_spectrum_create does (same codes and messages), then wf: FMR_ERR_BAD_ARG (before the device
 * is opened; fmr_last_error names the field) for segments_per_line outside 1 .. 65536, max_lines < 1, an unknown which,
 * a struct_size larger than this library's, or n_rows x max_lines x fft_size x 4 bytes above 1 GiB; FMR_ERR_NO_DEVICE
 * for a valid pair without a device. */
int fmr_spectrum_create_waterfall(const fmr_spectrum_config *cfg, size_t cfg_size, const fmr_waterfall_config *wf,
                                  size_t wf_size, fmr_spectrum **out);
/* Synchronises; copies the oldest unread complete lines of `row` to out (up to cap_lines of them, N floats each) and
 * their c_l to counted (may be NULL), marks them read and returns how many it copied.  cap_lines = 0 returns the number
 * ready and copies nothing.  Each row has its own read position.  FMR_ERR_BAD_ARG for an object without a waterfall. */
int fmr_spectrum_read_waterfall(fmr_spectrum *s, int row, float *out, uint32_t *counted, size_t cap_lines,
                                fmr_waterfall_info *info);
/* Host only (no device).  psd: fft_size doubles in the layout above.  Keeps f_c when snr_db >= threshold_db and its band
 * power is >= that of every candidate f' with 0 < |f' - f_c| < bandwidth_hz (a tie goes to the lower frequency).
 * Writes up to cap stations in ascending offset order and returns how many there are (possibly more than cap);
 * FMR_ERR_BAD_ARG for raster_hz <= 0, bandwidth_hz <= 0, floor_percentile outside [0, 100), an invalid fft_size or
 * input_rate. */
int fmr_find_stations(const double *psd, int fft_size, double input_rate, const fmr_station_rule *rule, fmr_station *out,
                      int cap);

/* --- Modulation monitor (no counterpart in the reference).  An FM chain with the monitor enabled
 * measures the 384 kHz MPX of every stream / bank channel where it lies on the device: peak deviation and its
 * distribution (ITU-R SM.1268), MPX power (ITU-R BS.412), pilot and RDS injection, the noise above the multiplex.  The
 * audio, fmr_status, PPS events and RDS groups of the chain are what they are without it: the stage only reads the MPX.
 * Indices are absolute, counted from the chain's first MPX sample; nothing depends on the cut into blocks and calls.
 *   F = 384000, N = 1024, H = 512, M = interval_samples.  Record i covers the MPX samples [i M, (i + 1) M).
 * Time-domain part, over the finite samples x of the record (a non-finite sample is counted in n_nonfinite and enters
 * nothing else): n_finite; min and max (the samples' own fp32 values; both 0 when n_finite = 0); sum and sumsq (fp64 sums
 * of the fp32 samples and of their fp64 squares); a histogram of B = hist_bins uint32 counters over [-R, R), R =
 * hist_range (1.0 = 75 kHz): a sample's bin is clamp(floorf((x + Rf) * scale), 0, B - 1) with Rf = (float)R and
 * scale = (float)(B / (2 R)), all unfused fp32 (numpy float32 gives the same bin for every sample); samples beyond the
 * range land in the end bins.
 * Spectral part: segment j covers [j H, j H + N) and belongs to record floor(j H / M) (the last segment of a record
 * reaches 512 samples into the next record).  Periodic Hann window, built in double and rounded once to fp32.  One-sided
 * density, k = 0 .. 512 (bin k at k F / N Hz):  P_j[k] = c_k |sum_n w[n] x[j H + n] exp(-2 pi i k n / N)|^2 / (F sum w^2),
 * c_k = 2 for 0 < k < 512 and 1 at both ends, so that sum_k psd[k] F / N is the mean square.  A segment that holds a
 * non-finite sample is skipped and counted in segments_skipped; psd is the mean of the counted P_j (fp64 sum on the
 * device, divided on the host when read), all zeros when segments = 0.
 * Completion: record i is complete in the call that delivers the absolute sample (i + 1) M + 511, the last sample of
 * its last segment.
 * Ring: max_records = L records per stream.  When L unread records exist and another completes, the oldest is
 * overwritten and counted in records_dropped; processing never fails because of it.
 * Reproducibility: counts, histogram, min, max, segments and segments_skipped are bit-identical for any cut of the
 * input into calls; sum, sumsq and psd add the same fp32 per-segment values in fp64 in a fixed order without float atomics
 * (the same cut gives the same bits; another cut differs at fp64 rounding, ~1e-15 relative). */
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_monitor_config) as the caller knows it (0: cfg_size); a larger size is refused */
  uint32_t interval_samples;  /* M: a multiple of 512 in 512 .. 2^30; 0 = 384000 (one second) */
  int hist_bins;              /* B: 2 .. 1024; 0 = 256 */
  double hist_range;          /* R > 0, finite; 0 = 2.0 */
  int max_records;            /* L: 1 .. 4096; 0 = 64 */
} fmr_monitor_config;
typedef struct {
  uint64_t index, first_sample;   /* i and i M */
  uint32_t n_finite, n_nonfinite, segments, segments_skipped;
  float min, max;
  double sum, sumsq;
} fmr_monitor_record;
typedef struct {
  unsigned struct_size;
  int hist_bins, psd_bins;        /* B; 513 */
  uint64_t records_complete;      /* since create (of every stream: they run in step) */
  uint64_t records_dropped;       /* of this stream: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint32_t interval_samples;      /* M, B's range and L as enabled (defaults filled in) */
  int max_records;
  double hist_range;
  double bin_hz;                  /* F / N = 375 */
} fmr_monitor_info;
typedef struct {
  unsigned struct_size;
  int reserved;
  double tuning_offset_hz;        /* 75000 mean */
  double peak_deviation_hz;       /* 75000 max(max - mean, mean - min) */
  double rms;                     /* sqrt(var), MPX units */
  double mpx_power_dbr;           /* 10 log10(2 (75/19)^2 var): 0 dBr is a sine of +-19 kHz (BS.412); -INFINITY when var <= 0 */
  double pilot_deviation_hz;      /* 75000 sqrt(2 B(17875, 20125)) */
  double rds_deviation_hz;        /* 75000 sqrt(2 B(54600, 59400)): the unmodulated carrier of the same band power */
  double hf_noise_density;        /* mean psd[k] over 100 kHz <= k F / N <= 150 kHz, MPX^2 / Hz */
  uint64_t n_finite, segments;    /* pooled */
} fmr_monitor_levels;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG; any FMR_MODE_FM chain is accepted (fmr_create and fmr_create_rds,
 * banks, either resampler class, pipelined or in_order, -f, the equaliser); every other mode and front-end-only chains
 * are FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's first sample: a second call, or one after any processing
 * call, is FMR_ERR_BAD_ARG.  A chain that never calls it allocates nothing for the monitor and runs none of its kernels. */
int fmr_enable_monitor(fmr_chain *c, const fmr_monitor_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of `stream`, oldest first, and returns how
 * many: recs[cap], hist[cap x B] and psd[cap x 513] (either may be NULL).  cap = 0 returns the number waiting and drains
 * nothing.  info (may be NULL) takes info_size bytes (0 = this header's size).  FMR_ERR_BAD_ARG on a chain without the
 * monitor. */
int fmr_monitor_read(fmr_chain *c, int stream, fmr_monitor_record *recs, uint32_t *hist, double *psd, int cap,
                     fmr_monitor_info *info, size_t info_size);
/* Host only, in double, no device.  Pools n records (psd: n x 513 as read, or NULL: the band levels are 0): sums and
 * counts add, min and max run over the records with n_finite > 0, psd is weighted by segments.  With mean = sum / n_finite,
 * var = sumsq / n_finite - mean^2 and B(lo, hi) = sum of psd[k] F / N over lo <= k F / N <= hi it fills the levels above
 * (n_finite = 0: mean, var and the peak deviation are 0). */
int fmr_monitor_derive(const fmr_monitor_record *recs, const double *psd, int n, fmr_monitor_levels *out, size_t out_size);

/* --- Audio monitor: a level meter on the decoded audio, the other half of a broadcast monitor.
 * An FM chain with it enabled measures the finished audio of every stream / bank channel where the output mux wrote it
 * on the device: programme loudness (ITU-R BS.1770-4 / EBU R 128), sample and true peak, stereo correlation, silence.
 * The audio, fmr_status, PPS events, RDS groups and modulation-monitor records of the chain are what they are without
 * it: the stage only reads the audio.  The AM family (and NBFM) is out of scope: FMR_MODE_FM chains only.
 * Indices are absolute audio sample indices per stream, counted from the chain's first audio sample; nothing depends
 * on the cut into blocks and calls.  ch = 2 for a stereo chain (its audio is interleaved L/R doubles, also when the
 * station is mono and L = R), ch = 1 for stereo = 0.  A non-finite audio sample is counted in n_nonfinite (once per
 * channel value) and enters everything below as 0.0.
 * K-weighting (BS.1770-4, 48 kHz), two biquads in the form w = x - a1 w1 - a2 w2; y = b0 w + b1 w1 + b2 w2:
 *   stage 1: b = 1.53512485958697, -2.69169618940638, 1.19839281085285; a = 1, -1.69065929318241, 0.73248077421585
 *   stage 2: b = 1, -2, 1;                                              a = 1, -1.99004745483398, 0.99007225036621
 * fp64, unfused, evaluated left to right, state zero at the chain's first sample and carried on the device across calls.
 * (A 0 dBFS 997 Hz sine in one channel reads -3.01 LKFS; the coefficients are used as they are at every output rate.)
 * Sub-block q covers the samples [q Q, (q + 1) Q), Q = step_samples.  Its record holds, per channel c:
 *   kw_sumsq[c]    sum of the squared K-weighted samples;   sumsq[c]  sum x^2;   sum_lr  sum L R (0 when ch = 1);
 *   sample_peak[c] max |x|, the sample's own value;
 *   true_peak[c]   max over n in the sub-block and p = 0 .. 3 of |y[n, p]|, a 4x interpolator with an identity phase:
 *                  y[n, p] = sum_{k = -5 .. 6} x[n - 6 + k] g_p[k],  g_p[k] = sinc(k - p/4) (0.5 + 0.5 cos(pi (k - p/4) / 6)),
 *                  summed with k ascending, samples before index 0 being 0, and y[n, 0] = x[n - 6] itself.  It is a
 *                  causal 12-tap polyphase filter reaching 11 samples back: a sub-block needs no future sample.  (A unit
 *                  sine at fs/4 sampled at 45 degrees has sample peak 0.7071 and reads 0.9962.)
 * Channel-1 fields are 0 when ch = 1.
 * Completion: record q is complete in the call that delivers the sample (q + 1) Q - 1.
 * Ring: max_records = L records per stream.  When L unread records exist and another completes, the oldest is
 * overwritten and counted in records_dropped; processing never fails because of it.
 * Reproducibility: index, first_sample, n_nonfinite, channels, step_samples, sample_peak and true_peak are bit-identical
 * for any cut of the input into calls.  The sums are fp64 in a fixed order without float atomics (the same cut gives the
 * same bits; another cut differs at fp64 rounding: ~1e-15 relative for sumsq and sum_lr, and for kw_sumsq ~1e-13 of the
 * largest sub-block nearby, because the recurrence is restarted from chunk states). */
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_loudness_config) as the caller knows it (0: cfg_size); a larger size is refused */
  uint32_t step_samples;      /* Q: a multiple of 16 in 48 .. 2^20; 0 = 4800 (100 ms at 48 kHz) */
  int max_records;            /* L: 1 .. 65536; 0 = 1024 */
} fmr_loudness_config;
typedef struct {
  uint64_t index, first_sample;   /* q and q Q */
  uint32_t n_nonfinite, channels; /* ch */
  uint32_t step_samples, reserved;/* Q, so that a record can be derived from by itself */
  double kw_sumsq[2], sumsq[2], sum_lr, sample_peak[2], true_peak[2];
} fmr_loudness_record;
typedef struct {
  unsigned struct_size;
  int channels;                   /* ch */
  uint64_t records_complete;      /* since create (of every stream: they run in step) */
  uint64_t records_dropped;       /* of this stream: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint32_t step_samples;          /* Q and L as enabled (defaults filled in) */
  int max_records;
} fmr_loudness_info;
typedef struct {
  unsigned struct_size;
  int reserved;
  double momentary_lufs, momentary_max_lufs;      /* the last window that exists and the maximum; -INFINITY when none */
  double short_term_lufs, short_term_max_lufs;
  double integrated_lufs;                         /* -INFINITY when no window passes the absolute gate */
  double sample_peak_dbfs, true_peak_dbtp;        /* 20 log10 of the largest peak of all records; -INFINITY for 0 */
  double correlation;                             /* sum LR / sqrt(sum L^2 sum R^2); 0 when the denominator is 0 */
  double side_to_mid_db;                          /* +-INFINITY when mid / side is 0, 0 when both are */
  uint64_t longest_silence_blocks, trailing_silence_blocks;
  uint64_t n_nonfinite;                           /* pooled */
  uint64_t momentary_windows, gated_windows;      /* windows that exist; windows that pass both gates */
} fmr_loudness_levels;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG; any FMR_MODE_FM chain is accepted (fmr_create and fmr_create_rds,
 * banks, pipelined or in_order); every other mode and front-end-only chains are FMR_ERR_UNSUPPORTED.  Allowed once,
 * before the chain's first sample: a second call, or one after any processing call, is FMR_ERR_BAD_ARG.  A chain that
 * never calls it allocates nothing for the audio monitor and runs none of its kernels. */
int fmr_enable_loudness(fmr_chain *c, const fmr_loudness_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of `stream`, oldest first, and returns how
 * many.  cap = 0 returns the number waiting and drains nothing.  info (may be NULL) takes info_size bytes (0 = this
 * header's size).  FMR_ERR_BAD_ARG on a chain without the audio monitor. */
int fmr_loudness_read(fmr_chain *c, int stream, fmr_loudness_record *recs, int cap, fmr_loudness_info *info, size_t info_size);
/* Host only, in double, no device.  n records in ascending order as read.  Windows are built only over records with
 * consecutive index: a gap left by dropped records breaks windows and silence runs.  With Q = step_samples and
 *   Z_i = sum_c sum_{j = i - 3 .. i} kw_sumsq_c[j] / (4 Q),  momentary = -0.691 + 10 log10 Z_i  (-INFINITY for Z = 0),
 * short-term the same over 30 sub-blocks.  integrated_lufs gates all momentary windows as BS.1770-4 does: the absolute
 * gate -70, then the relative gate 10 LU under the loudness of the mean Z of the windows that passed the absolute one;
 * the loudness of the mean Z of what passes both.  correlation and side_to_mid_db = 10 log10((sum L^2 + sum R^2 -
 * 2 sum LR) / (sum L^2 + sum R^2 + 2 sum LR)) pool all records.  A sub-block is silent when (sumsq_0 + sumsq_1) / (ch Q) <
 * 10^(silence_dbfs / 10); longest_silence_blocks is the longest run of consecutive silent sub-blocks,
 * trailing_silence_blocks the run that ends at the last record.  Loudness range (EBU 3342) is not computed. */
int fmr_loudness_derive(const fmr_loudness_record *recs, int n, double silence_dbfs, fmr_loudness_levels *out, size_t out_size);

/* --- Weak-signal handling: what every FM receiver does to a station near the FM threshold --
 * stereo blend, high cut and soft mute -- driven by the ultrasonic noise of the station's own MPX.  The stage is off by
 * default and absent when off; the reference has no weak-signal logic, so parity with it is a matter of chains without the
 * stage.  In FMR_WS_MEASURE the stage only reads: audio, fmr_status, PPS events, RDS groups and every monitor's records are
 * what they are without it.  In FMR_WS_ACT it rewrites the finished audio behind the output mux, in front of the audio
 * monitor, the analyser and the output stage: they and the caller get the handled audio.
 * Timeline: the MPX has F = 384000 and absolute sample indices from the chain's first MPX sample; samples in front of
 * index 0 are 0.  A control interval is Q = 768 MPX samples (2 ms); interval j covers [j Q, (j + 1) Q).  The audio has
 * 48000 frames per second and absolute frame indices; an audio interval is A = 96 frames.
 * Detector (ultrasonic noise): h is a 63-tap linear-phase high-pass built on the host in double,
 *   lp[k] = 2 fc sinc(2 fc (k - 31)) w[k],  fc = 110000 / F,  w[k] = 0.42 - 0.5 cos(2 pi k / 62) + 0.08 cos(4 pi k / 62),
 *   lp scaled to sum 1,  h = delta[k - 31] - lp        (sinc(x) = sin(pi x) / (pi x); fmr_filter_table("ws_usn"))
 * (DC gain -2e-16, at most -75 dB up to 90 kHz, within +-0.015 dB from 125 kHz up: programme, pilot and RDS lie below
 * 60 kHz, what is left is discriminator noise).  y[n] = sum_k h[k] (double)x[n - k] with x the chain's fp32 MPX, k
 * ascending, in fp64; u_j = (sum of y[n]^2 over interval j) / Q.  A non-finite x is counted in n_nonfinite and enters as 0.
 * Control, per stream, serial in j, in fp64, carried on the device across calls:
 *   s_j = s_{j-1} + c (u_j - s_{j-1}),  c = the attack coefficient when u_j > s_{j-1}, else the release coefficient,
 *   coefficient = 1 - exp(-2 / tau_ms) (computed on the host),  s_{-1} = 0;
 *   D_j = 10 log10(s_j) in dB re full-scale MPX^2 (full-scale MPX = 1.0 = 75 kHz; -INFINITY for s_j = 0);
 *   per action a: t_a(j) = clamp((D_j - lo_a) / (hi_a - lo_a), 0, 1); 0 for -INFINITY and for an action switched off.
 * Action: audio frame f uses the control values of interval J = floor(f / A) - 1 and ramps to them from those of J - 1:
 *   p = ((f mod A) + 1) / A,  v(f) = v_{J-1} + p (v_J - v_{J-1}) for each of the three t; intervals below 0 hold 0.
 * (Interval J is complete when frame f exists: the audio resampler delivers frame f only after MPX sample 8 f.)  Then, in
 * fp64, unfused, in this order, with L = R = x on a stereo = 0 chain, which skips steps 1 and 2:
 *   1. S = 0.5 (L - R)                2. L1 = L - t_b S,  R1 = R + t_b S
 *   3. w[f] = w[f - 1] + alpha (x1[f] - w[f - 1]) per channel,  alpha = 1 - exp(-2 pi highcut_hz / 48000),  w[-1] = 0
 *   4. x2 = x1 + t_h (w - x1)         5. out = (1 - t_m (1 - g_floor)) x2,  g_floor = 10^(mute_floor_db / 20)
 * With all three t at 0 every step returns its input bit for bit on finite audio: a clean station's audio is unchanged.
 * The high cut is a crossfade to a fixed one-pole low-pass, so its recurrence is time-invariant.
 * Records: record i covers the intervals [i R, (i + 1) R), R = record_intervals, and is complete in the call that delivers
 * MPX sample (i + 1) R Q - 1.  usn_sum = sum of u_j, usn_peak = max u_j, smoothed = s at the record's end, t_* the three
 * t at its end, max_* their maxima over the record.  Ring, drop counting and info as for the audio monitor.
 * Reproducibility: the integer fields are bit-identical for any cut of the input into calls; the doubles agree between
 * cuts at fp64 rounding (u within 1e-12 of mean_n (sum_k |h_k| |x_{n-k}|)^2); the same cut gives the same bits; no float
 * atomics.
 * Default thresholds, in dB of s: the steady detector reading of the benchmark's station at an IF C/N (in 384 kHz) of 30,
 * 20, 12 and 6 dB, measured on the float64 oracle's MPX (DESIGN.md section 16 has the table): blend -33 .. -23, high cut
 * -23 .. -15, mute -15 .. -9. */
enum { FMR_WS_MEASURE = 0, FMR_WS_ACT = 1 };
enum { FMR_WS_BLEND = 1, FMR_WS_HIGHCUT = 2, FMR_WS_MUTE = 4 };
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_weak_signal_config) as the caller knows it (0: cfg_size); a larger size is refused */
  int mode;                   /* FMR_WS_MEASURE (the audio is never written) | FMR_WS_ACT */
  unsigned actions;           /* FMR_WS_BLEND | FMR_WS_HIGHCUT | FMR_WS_MUTE; 0 = all three */
  int record_intervals;       /* R: 1 .. 1000; 0 = 50 (100 ms) */
  int max_records;            /* L: 1 .. 65536; 0 = 1024 */
  int reserved;
  double attack_ms, release_ms;            /* > 0 .. 60000; 0 = 10 and 500 */
  double blend_lo_db, blend_hi_db;         /* lo < hi, finite; both 0 = the defaults above */
  double highcut_lo_db, highcut_hi_db;
  double mute_lo_db, mute_hi_db;
  double highcut_hz;                       /* 500 .. 15000; 0 = 2500 */
  double mute_floor_db;                    /* < 0 and finite; 0 = -20 */
} fmr_weak_signal_config;
typedef struct {
  uint64_t index, first_interval;          /* i and i R */
  uint32_t n_intervals, n_nonfinite;       /* R; non-finite MPX samples of the record */
  double usn_sum, usn_peak, smoothed;
  double t_blend, t_highcut, t_mute;
  double max_blend, max_highcut, max_mute;
} fmr_weak_signal_record;
typedef struct {
  unsigned struct_size;
  int channels;                   /* 2 for a stereo chain, 1 for stereo = 0 */
  uint64_t records_complete;      /* since create (of every stream: they run in step) */
  uint64_t records_dropped;       /* of this stream: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint64_t intervals_complete;    /* control intervals complete since create */
  int record_intervals, max_records;   /* R and L as enabled (defaults filled in) */
  int mode;
  unsigned actions;
} fmr_weak_signal_info;
typedef struct {
  unsigned struct_size;
  int reserved;
  double usn_mean_db, usn_peak_db;         /* 10 log10 of (sum usn_sum / sum n_intervals) and of max usn_peak; -INFINITY for 0 */
  double usn_mean_hz, usn_peak_hz;         /* 75000 sqrt of the same: RMS deviation of the ultrasonic noise */
  double blend_share, highcut_share, mute_share;   /* sum n_intervals of the records with max_* > 0 / sum n_intervals */
  double t_blend, t_highcut, t_mute;       /* of the last record */
  uint64_t n_intervals, n_nonfinite;       /* pooled */
} fmr_weak_signal_levels;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG; any FMR_MODE_FM chain is accepted (stereo or stereo = 0, banks,
 * fmr_create_rds, either resampler class, pipelined or in_order, the equaliser); every other mode, front-end-only chains
 * and channelizers, and a chain with pilot_shift (its two channels are not L and R) are FMR_ERR_UNSUPPORTED.  Allowed
 * once, before the chain's first sample: a second call, or one after any processing call, is FMR_ERR_BAD_ARG.  A chain that
 * never calls it allocates nothing for the stage and launches none of its kernels. */
int fmr_enable_weak_signal(fmr_chain *c, const fmr_weak_signal_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of `stream`, oldest first, and returns how
 * many.  cap = 0 returns the number waiting and drains nothing.  info (may be NULL) takes info_size bytes (0 = this
 * header's size).  FMR_ERR_BAD_ARG on a chain without the stage. */
int fmr_weak_signal_read(fmr_chain *c, int stream, fmr_weak_signal_record *recs, int cap, fmr_weak_signal_info *info,
                         size_t info_size);
/* Host only, in double, no device: pools n records (n >= 1, each with n_intervals > 0) into the levels above. */
int fmr_weak_signal_derive(const fmr_weak_signal_record *recs, int n, fmr_weak_signal_levels *out, size_t out_size);

/* --- Impulse blanker on the capture: ignition, switching supplies, lightning, ADC glitches and
 * dropped packets are one or two samples long in the wideband capture; the front end spreads each over its 103 + 210
 * taps.  The stage zeroes them in the input rows of a call before any front-end form reads them.  It is off by default
 * and absent when off.  In FMR_NB_MEASURE it only reads: every output of the chain is what it is without the stage.  In
 * FMR_NB_ACT every reader of the call's input (every front-end form, the input history on whichever stream it is
 * carried over, a bank's one-row history) reads the blanked rows, which the stage keeps in buffers of its own: the
 * caller's buffer is never written.
 * Timeline: per input row, sample index n counts from the chain's first sample, across blocks and calls of any length.
 * Interval j covers [j Q, (j + 1) Q), Q = 4096.
 * Power: p[n] = fl32(fl32(re re) + fl32(im im)), unfused.  A non-finite p (NaN or Inf) makes the sample non-finite.
 * Level (exact: any cut into calls and any summation order gives the same bits): q[n] = 0 for a non-finite sample, else
 * floor(min(p[n], 256) 2^36) as a 64-bit integer; A_j = sum of q[n] over interval j (below 2^56).
 * Threshold (no recurrence): W = average_intervals, g = 10^(threshold_db / 10) and r[c] = 1 / (c 2^48), c = 1 .. W, are
 * computed on the host in double.  T_0 = +INFINITY.  For j >= 1: c = min(j, W), S = A_{j-c} + .. + A_{j-1} (integer),
 * T_j = max(g ((double)S r[c]), 2^-30): two fp64 products in this order.
 * Trigger: trig[n] = non-finite[n] or (double)p[n] > T_{floor(n / Q)}.
 * Gate, G = gate_samples: gate[n] = some trig[i], i in [max(0, n - G + 1), n].  Causal: the first sample over the
 * threshold is itself gated, nothing in front of it is; a call boundary decides nothing.
 * Give-up, M = max_run_samples: blank[n] = gate[n] and some i in [n - M, n - 1] with i < 0 or not gate[i].  A gate that
 * stays closed longer than M samples passes its input through again until it has opened once: a +20 dB level step
 * zeroes M samples, not everything until the average has caught up, and a run of non-finite samples longer than M
 * passes through as it is.  blank[n] depends on the samples n - (G - 1 + M) .. n only.
 * Output: out[n] = (0, 0) where blank[n], else x[n] bit for bit.
 * Records: record i covers the intervals [i R, (i + 1) R), R = record_intervals, and is complete in the call that
 * delivers sample (i + 1) R Q - 1.  n_runs counts the samples with blank[n] and not blank[n - 1]; power_q = sum of
 * (A_j >> 12); peak = the largest finite p; threshold = T of the record's last interval.  Every field is bit-identical
 * for any cut of the input into blocks and calls.  Ring, drop counting and info as for the audio monitor. */
enum { FMR_NB_MEASURE = 0, FMR_NB_ACT = 1 };
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_blanker_config) as the caller knows it (0: cfg_size); a larger size is refused */
  int mode;                   /* FMR_NB_MEASURE (default) | FMR_NB_ACT */
  double threshold_db;        /* 6 .. 40; 0 = 12 */
  int gate_samples;           /* G: 1 .. 256; 0 = max(2, ceil(0.8e-6 input_rate)): 8 at 10 MS/s, 2 at 2.5 MS/s */
  int max_run_samples;        /* M: G .. 1024 with G - 1 + M <= Q; 0 = 8 G */
  int average_intervals;      /* W: 1 .. 64; 0 = 16 (6.6 ms at 10 MS/s) */
  int record_intervals;       /* R: 1 .. 4096; 0 = 256 */
  int max_records;            /* L: 1 .. 65536; 0 = 1024 */
  int reserved;
} fmr_blanker_config;
typedef struct {
  uint64_t index, first_interval;          /* i and i R */
  uint64_t n_triggers, n_blanked, n_nonfinite, n_runs;
  uint64_t power_q;
  double threshold;
  uint32_t n_intervals;                    /* R */
  float peak;
} fmr_blanker_record;
typedef struct {
  unsigned struct_size;
  int rows;                       /* input rows of the chain: 1 for a bank or a channelizer */
  uint64_t records_complete;      /* since create (of every row: they run in step) */
  uint64_t records_dropped;       /* of this row: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint64_t intervals_complete;    /* intervals complete since create */
  int mode, gate_samples, max_run_samples, average_intervals, record_intervals, max_records;   /* as enabled (defaults filled in) */
} fmr_blanker_info;
typedef struct {
  unsigned struct_size;
  int reserved;
  double blanked_share;           /* sum n_blanked / (sum n_intervals Q) */
  double runs_per_second;         /* sum n_runs input_rate / (sum n_intervals Q), input_rate being fmr_blanker_derive's argument */
  double level_dbfs;              /* 10 log10(sum power_q / (sum n_intervals 2^36)): mean |x|^2 re full scale 1.0; -INFINITY for 0 */
  double peak_dbfs;               /* 10 log10(max peak); -INFINITY for 0 */
  uint64_t n_intervals, n_triggers, n_blanked, n_nonfinite, n_runs;   /* pooled */
} fmr_blanker_levels;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG.  Accepted is every chain that runs the IF resampler on FMR_IQ_CF32
 * input: plain chains of any mode, with or without enable_fourth_down, banks (one row serves all channels),
 * channelizers and front-end-only chains, either resampler class, pipelined or in_order, through every processing entry
 * point.  Raw input formats and chains without the resampler are FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's
 * first sample: a second call, or one after any processing call, is FMR_ERR_BAD_ARG.  A failed call leaves the chain and
 * fmr_debug_live_resources as they were. */
int fmr_enable_blanker(fmr_chain *c, const fmr_blanker_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of input row `row` (0 for a bank), oldest
 * first, and returns how many.  cap = 0 returns the number waiting and drains nothing.  info (may be NULL) takes info_size
 * bytes (0 = this header's size).  FMR_ERR_BAD_ARG on a chain without the stage. */
int fmr_blanker_read(fmr_chain *c, int row, fmr_blanker_record *recs, int cap, fmr_blanker_info *info, size_t info_size);
/* Host only, in double, no device: pools n records (n >= 1, each with n_intervals > 0) into the levels above.  input_rate
 * (samples per second, > 0) is only used for runs_per_second. */
int fmr_blanker_derive(const fmr_blanker_record *recs, int n, double input_rate, fmr_blanker_levels *out, size_t out_size);

/* --- DC-offset and IQ-imbalance correction on the capture: a direct-conversion SDR adds a carrier
 * at 0 Hz and mirrors every station at +f onto -f, 25 to 40 dB down.  A single-station chain does not mind; a bank, a
 * channelizer, the band spectrum and the station finder see the carrier as a station and a strong station's image on
 * another raster point.  The stage estimates both errors from the capture itself and removes them in the input rows of a
 * call, ahead of the blanker and of every front-end form.  It is off by default and absent when off.  In FMR_IQC_MEASURE
 * it only reads: every output of the chain is what it is without the stage.  In FMR_IQC_ACT every reader of the call's
 * input (the blanker first, when there is one) reads the corrected rows, which the stage keeps in buffers of its own: the
 * caller's buffer is never written.
 * Everything below applies per input row.  Sample index n counts from the chain's first sample, across blocks and calls
 * of any length.
 * Interval: interval j covers [j Q, (j + 1) Q), Q = 4096 (the blanker's).
 * Usable sample: p = fl32(fl32(re re) + fl32(im im)), unfused.  A sample is non-finite if either component is NaN or Inf.
 * It is usable if it is finite and p <= 4: anything more than 6 dB over full scale is an impulse or a mis-scaled capture,
 * contributes to no sum and is counted (n_skipped).
 * Moments (exact integers: any cut into calls and any summation order gives the same bits): for a usable sample
 * a_r = floor(re 2^36), a_i = floor(im 2^36), a_rr = floor(fl32(re re) 2^36), a_ii = floor(fl32(im im) 2^36),
 * a_ri = floor(fl32(re im) 2^36), signed 64-bit, floor towards -INFINITY, the float widened to double first.  Per
 * interval: N_j (usable samples), S_r, S_i, S_rr, S_ii, S_ri.  With W <= 1024 a window sum stays below 2^60.
 * Window: W = average_intervals.  For interval j, c = min(j, W); the window is the intervals j - c .. j - 1: strictly
 * past, so a call boundary decides nothing.  Window sums are differences of running 64-bit totals (wrap-around is
 * harmless).
 * Coefficients of interval j, in fp64, each operation rounded once, in this order.  If c = 0 or the window's N < Q / 2:
 * d = 0, w = 0.  Otherwise r = 1 / ((double)N 2^36); m_r = (double)S_r r, m_i likewise; E_rr = (double)S_rr r, E_ii and
 * E_ri likewise; P = (E_rr + E_ii) - (m_r m_r + m_i m_i); C_r = (E_rr - E_ii) - (m_r m_r - m_i m_i);
 * C_i = 2 E_ri - 2 (m_r m_i); D = P P - (C_r C_r + C_i C_i).  If !(P > 2^-40) or !(D > 0): w = 0.  Else t = P + sqrt(D),
 * w_r = C_r / t, w_i = C_i / t: the exact root of E[y^2] = 0 for y = z - w conj(z), to first order C / 2P.  If
 * w_r w_r + w_i w_i > 1/16: w = 0 and the interval counts as refused -- an image less than 12 dB down is not receiver
 * mismatch but an improper signal (a real-valued capture, an AM carrier at 0 Hz).  d = (m_r, m_i).  `correct` selects
 * what is applied (FMR_IQC_DC | FMR_IQC_BALANCE; 0 = both); the part not selected is set to 0.  The applied coefficients
 * are then rounded to fp32: dr, di, wr, wi.
 * Output: a non-finite sample passes bit for bit (the blanker behind the stage still sees it).  A sample of an interval
 * whose four applied coefficients are all zero passes bit for bit.  Otherwise, in fp32, every product and sum rounded,
 * nothing fused: zr = re - dr, zi = im - di, yr = zr - fl32(fl32(wr zr) + fl32(wi zi)),
 * yi = zi - fl32(fl32(wi zr) - fl32(wr zi)).  Denormals follow IEEE.
 * Records: record i covers the intervals [i R, (i + 1) R), R = record_intervals, and is complete in the call that delivers
 * its last sample.  The sums are over the record's usable samples; n_refused counts intervals; dc_re .. w_im are the
 * applied coefficients of the record's last interval.  Every field is bit-identical for any cut of the input into
 * blocks and calls.  Ring, drop counting and info as for the blanker.
 * A station at offset 0 has its carrier notched (about input_rate / (W Q) wide): hence `correct`, and off by default.  A
 * capture not scaled to full scale 1.0 is skipped whole and passes unchanged. */
enum { FMR_IQC_MEASURE = 0, FMR_IQC_ACT = 1 };
enum { FMR_IQC_DC = 1, FMR_IQC_BALANCE = 2 };
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_iq_correction_config) as the caller knows it (0: cfg_size); a larger size is refused */
  int mode;                   /* FMR_IQC_MEASURE (default) | FMR_IQC_ACT */
  int correct;                /* FMR_IQC_DC | FMR_IQC_BALANCE; 0 = both */
  int average_intervals;      /* W: 1 .. 1024; 0 = 64 (105 ms at 2.5 MS/s) */
  int record_intervals;       /* R: 1 .. 4096; 0 = 256 */
  int max_records;            /* L: 1 .. 65536; 0 = 1024 */
  int reserved;
} fmr_iq_correction_config;
typedef struct {
  uint64_t index, first_interval;          /* i and i R */
  uint64_t n_usable, n_nonfinite, n_skipped, n_refused;
  int64_t sum_re, sum_im, sum_rr, sum_ii, sum_ri;
  uint32_t n_intervals;                    /* R */
  float dc_re, dc_im, w_re, w_im;
  uint32_t reserved;
} fmr_iq_correction_record;
typedef struct {
  unsigned struct_size;
  int rows;                       /* input rows of the chain: 1 for a bank or a channelizer */
  uint64_t records_complete;      /* since create (of every row: they run in step) */
  uint64_t records_dropped;       /* of this row: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint64_t intervals_complete;    /* intervals complete since create */
  int mode, correct, average_intervals, record_intervals, max_records;   /* as enabled (defaults filled in) */
  int reserved;
} fmr_iq_correction_info;
typedef struct {
  unsigned struct_size;
  int refused;                    /* 1: the pooled sums give an image less than 12 dB down, w is reported as 0 */
  double dc_re, dc_im;            /* d from the pooled sums (0 when fewer than Q / 2 usable samples) */
  double dc_dbfs;                 /* 20 log10 |d|; -INFINITY for 0 */
  double w_re, w_im;
  double image_rejection_db;      /* -20 log10 |w|: of the uncorrected capture; +INFINITY for 0 */
  double gain_imbalance_db;       /* 20 log10 |rho|, rho = (1 - w) / (1 + w): inverts "I exact, Q' = g (Q cos phi + I sin phi)" */
  double phase_error_deg;         /* -arg rho */
  double usable_share;            /* sum n_usable / (sum n_intervals Q) */
  uint64_t n_intervals, n_usable, n_nonfinite, n_skipped, n_refused;   /* pooled */
} fmr_iq_correction_levels;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG.  Accepted is every chain that runs the IF resampler on FMR_IQ_CF32
 * input, of any mode and shape (as fmr_enable_blanker).  Raw input formats and chains without the resampler are
 * FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's first sample, before or after fmr_enable_blanker: a second
 * call, or one after any processing call, is FMR_ERR_BAD_ARG.  A failed call leaves the chain and
 * fmr_debug_live_resources as they were. */
int fmr_enable_iq_correction(fmr_chain *c, const fmr_iq_correction_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of input row `row` (0 for a bank), oldest
 * first, and returns how many.  cap = 0 returns the number waiting and drains nothing.  info (may be NULL) takes info_size
 * bytes (0 = this header's size).  FMR_ERR_BAD_ARG on a chain without the stage. */
int fmr_iq_correction_read(fmr_chain *c, int row, fmr_iq_correction_record *recs, int cap, fmr_iq_correction_info *info,
                           size_t info_size);
/* Host only, in double, no device: pools n records (n >= 1, each with n_intervals > 0) and recomputes d and w from the
 * pooled sums with the formulas above (both parts, whatever `correct` was). */
int fmr_iq_correction_derive(const fmr_iq_correction_record *recs, int n, fmr_iq_correction_levels *out, size_t out_size);

/* --- Audio analyser: the spectrum analyser the reference's author judges receivers with, on the
 * device.  A decoder chain of any mode with it enabled measures the finished audio of every stream / bank channel where
 * the output mux wrote it: the level and frequency of a test tone, THD, THD+N, SINAD and the noise floor, per channel or
 * in the mid / side view.  The audio, fmr_status, PPS events, RDS groups, every monitor's records and the output PCM of
 * the chain are what they are without it: the stage only reads the audio.
 * Input: 48 kHz doubles, a frame being one sample per channel; ch = 2 for a stereo chain (interleaved L/R), otherwise 1.
 * Indices are absolute frame indices per stream, counted from the chain's first audio frame; nothing depends on the cut
 * into blocks and calls.
 *   N = fft_size, H = N / 2, M = interval_samples (a multiple of H).  Segment j covers the frames [j H, j H + N) and is
 * processed in the call that delivers its last frame; record i covers [i M, (i + 1) M); segment j belongs to record
 * floor(j H / M) (a record holds M / H segments, its last one reaches H frames into the next record).
 * Time-domain part of a record, over the first H frames of each of its segments (every frame enters once): sum[c] and
 * sumsq[c], fp64 sums of the samples and of their squares; a non-finite sample is counted in n_nonfinite (once per
 * channel value) and enters as 0.0.  Channel-1 fields are 0 when ch = 1.
 * Spectral part of a segment: each sample is rounded once to fp32 and multiplied by the fp32 window, the periodic 4-term
 * Blackman-Harris w[n] = 0.35875 - 0.48829 cos(2 pi n / N) + 0.14128 cos(4 pi n / N) - 0.01168 cos(6 pi n / N), built in
 * double and rounded once (the twiddles likewise).  One complex N-point FFT takes z[n] = wL[n] + i wR[n]; with X = Z[k]
 * and Y = conj Z[(N - k) mod N] the channels are L[k] = (X + Y) / 2 and R[k] = (X - Y) / (2 i), k = 0 .. N / 2.  A record
 * accumulates in fp64, over its counted segments, three rows of N / 2 + 1 bins: |L[k]|^2, |R[k]|^2 and
 * C[k] = Re(L[k] conj R[k]).  With ch = 1 the imaginary input is 0, the first row is |Z[k]|^2 and the other two are 0.
 * A segment that holds a sample which is not finite as fp32 is skipped for the spectral part and counted in `skipped`;
 * `segments` counts the others.
 * What fmr_analyser_read returns is scaled to POWER: row[k] c_k / (N sum w^2 segments), c_k = 2 for 0 < k < N / 2 and 1 at
 * both ends (all zeros when segments = 0): a sine of amplitude A at any frequency sums to A^2 / 2 over its main lobe
 * (+-4 bins), and white noise of variance v sums to v over all bins.
 * Completion: record i is complete in the call that delivers the frame (i + 1) M + H - 1, the last frame of its last
 * segment.
 * Ring: max_records = L records per stream.  When L unread records exist and another completes, the oldest is
 * overwritten and counted in records_dropped; processing never fails because of it.
 * Device memory: the ring takes n_streams L 3 (N / 2 + 1) 8 bytes (3.1 MB per stream at the defaults, 100 MB for a
 * 32-channel bank; 403 MB per stream at N = 8192 with L = 4096), the partial sums of a call up to 128 rows of
 * 3 (N / 2 + 1) doubles per stream more.  Size L for the reader's period.
 * Reproducibility: the integer fields are bit-identical for any cut of the input into calls; the sums add fixed
 * per-segment values in fp64 in a fixed order without float atomics (the same cut gives the same bits; another cut
 * differs at fp64 rounding). */
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_analyser_config) as the caller knows it (0: cfg_size); a larger size is refused */
  int fft_size;               /* N: 1024, 2048, 4096 or 8192; 0 = 4096 */
  uint32_t interval_samples;  /* M: a multiple of N / 2 in N / 2 .. 2^24; 0 = 6 N */
  int max_records;            /* L: 1 .. 4096; 0 = 64 */
} fmr_analyser_config;
typedef struct {
  uint64_t index, first_sample;   /* i and i M */
  uint32_t segments, skipped;     /* segments counted in the rows; segments skipped */
  uint32_t n_nonfinite, channels; /* ch */
  uint32_t fft_size, interval_samples;   /* N and M, so that records can be derived from by themselves */
  double sum[2], sumsq[2];
} fmr_analyser_record;
typedef struct {
  unsigned struct_size;
  int channels;                   /* ch */
  uint64_t records_complete;      /* since create (of every stream: they run in step) */
  uint64_t records_dropped;       /* of this stream: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint32_t interval_samples;      /* M, L and N as enabled (defaults filled in) */
  int max_records;
  int fft_size, bins;             /* N; N / 2 + 1 */
  double bin_hz;                  /* 48000 / N */
} fmr_analyser_info;
/* What to measure (every 0 is the default named). */
typedef struct {
  unsigned struct_size;
  int view;                       /* 0 = L (the only view of ch = 1 records), 1 = R, 2 = M: P = (P_L + P_R + 2 C) / 4,
                                     3 = S: P = max(0, (P_L + P_R - 2 C) / 4) */
  double band_lo_hz, band_hi_hz;  /* the measurement band: 0 = 20 and 0 = 15000; 0 <= lo < hi <= 24000 */
  double tone_hz;                 /* 0 = the strongest bin of the band; otherwise the strongest bin within +- tone_search_hz */
  double tone_search_hz;          /* 0 = 50 */
  int max_harmonic;               /* 2 .. 64; 0 = 10 */
  int reserved;                   /* must be 0 */
  double min_tone_dbfs;           /* a tone below it is none; 0 = -60 */
} fmr_analyser_rule;
typedef struct {
  unsigned struct_size;
  int tone_found;                 /* 0: tone_hz, tone_dbfs, thd, thd_n, sinad_db and harmonic_dbc are NaN, noise_dbfs is the whole band */
  double tone_hz;                 /* power centroid of the tone's lobe */
  double tone_dbfs;               /* 10 log10(2 P_t): a full-scale sine reads 0 */
  double thd;                     /* sqrt(P_h / P_t), a ratio (x 100 = per cent) */
  double thd_n;                   /* sqrt((P_h + P_n) / P_t) */
  double sinad_db;                /* 10 log10((P_t + P_h + P_n) / (P_h + P_n)); +INFINITY when P_h + P_n = 0 */
  double noise_dbfs;              /* 10 log10(2 P_n); -INFINITY for 0 */
  double band_dbfs;               /* 10 log10(2 P_band) */
  double harmonic_dbc[8];         /* 10 log10(P of harmonic h / P_t), h = 2 .. 9; NaN where the harmonic is not counted */
  double dc;                      /* mean of the view's samples: sum / frames (M and S: (sum_0 +- sum_1) / 2 / frames) */
  double total_dbfs;              /* 10 log10(2 sumsq / frames) of view L or R; NaN for M and S (the records hold no sum L R) */
  uint64_t segments, skipped, n_nonfinite;   /* pooled */
  int harmonics_counted, reserved;
} fmr_analyser_levels;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG; any chain with a decoder is accepted (every mode, banks, pipelined
 * or in_order); front-end-only chains (mode -1, channelizers) are FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's
 * first sample: a second call, or one after any processing call, is FMR_ERR_BAD_ARG.  A failed call leaves the chain as
 * it was.  A chain that never calls it allocates nothing for the analyser and runs none of its kernels. */
int fmr_enable_analyser(fmr_chain *c, const fmr_analyser_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of `stream`, oldest first, and returns how
 * many: recs[cap] and spectra[cap][3][N / 2 + 1], scaled to power as above (spectra may be NULL).  cap = 0 returns the
 * number waiting and drains nothing; since no more than max_records can wait, one call with cap = max_records drains
 * everything without asking first (every call synchronises the chain).  info (may be NULL) takes info_size bytes (0 = this header's size).
 * FMR_ERR_BAD_ARG on a chain without the analyser. */
int fmr_analyser_read(fmr_chain *c, int stream, fmr_analyser_record *recs, double *spectra, int cap,
                      fmr_analyser_info *info, size_t info_size);
/* Host only, in double, no device.  Pools the n records (spectra: n x 3 x (N / 2 + 1) as read) weighted by `segments`
 * (all zeros when no segment was counted); records of unlike fft_size or channels, n < 1, a view other than 0 on ch = 1
 * records and a rule field out of range are FMR_ERR_BAD_ARG (rule may be NULL: all defaults).
 * With bin k at k 48000 / N Hz, the band is the bins ceil(band_lo N / 48000) .. floor(band_hi N / 48000), B of them (at
 * least 9), P_band their sum, and W = 4 (the window's main lobe):
 *   k0 = the strongest bin of the band (tone_hz = 0) or of the band's bins within tone_hz +- tone_search_hz (the first of
 *   equals), clamped so that k0 - W .. k0 + W lie inside the band.  tone_found = 0 when there is no such bin, when
 *   k0 < 2 W + 1, or when 10 log10(2 P_t) < min_tone_dbfs, with P_t = sum of P[k] over |k - k0| <= W.
 *   tone_hz = (sum k P[k] / P_t) 48000 / N over the same bins.
 *   Harmonic h = 2 .. max_harmonic has its lobe at k_h = floor(h tone_hz N / 48000 + 0.5), bins k_h - W .. k_h + W; the
 *   first h whose lobe leaves the band ends the list.  A harmonic's power is the sum over those of its bins that no
 *   earlier lobe holds; P_h sums the harmonics, E counts the bins of all lobes, the tone's included.
 *   P_n = (P_band - P_t - P_h) B / (B - E)  (0 when B = E): the noise of the band's free bins (summed as such, not as
 *   the difference), spread over the band. */
int fmr_analyser_derive(const fmr_analyser_record *recs, const double *spectra, int n, const fmr_analyser_rule *rule,
                        size_t rule_size, fmr_analyser_levels *out, size_t out_size);

/* --- RF monitor (no counterpart in the reference).  An FM chain with it enabled measures the
 * received signal of every stream / bank channel where it lies on the device: level, C/N, the AM on the envelope
 * (multipath turns FM into AM: the 19 kHz line of the envelope is the classic indicator) and the depth of fades.  The
 * audio, fmr_status, PPS events, RDS groups and the records of both other monitors are what they are without it: the
 * stage only reads the call's IF ring slot.
 *   F = 384000, N = 1024, H = 512, M = interval_samples.  Indices are absolute, counted from the chain's first IF sample
 * (IF sample n and MPX sample n are the same instant); nothing depends on the cut into blocks and calls.
 * Signal: p[n], the squared magnitude of IF sample n as it enters the decoder: before the IF filter (-f), the IF AGC and
 * the equaliser; the signal fmr_status.if_rms is taken from.  Where the slot holds IF samples (re, im),
 * p = fl(fl(re re) + fl(im im)) in unfused fp32 (numpy float32 gives the same bits).  Behind a discriminator epilogue
 * (the fused front end and the R8B class without FMR_DEBUG_TAPS: the production path at 10 MS/s) the front end stored
 * |x|^2 there instead of the IF samples, and p is that float as stored.  The two forms may differ in the last bits of p:
 * the epilogue rounds its IF samples and their squares in its own order.
 * Time-domain part of record i, over [i M, (i + 1) M): a non-finite p is counted in n_nonfinite and enters nothing else;
 * n_finite; p_min and p_max (fp32, both 0 when n_finite = 0); m2 = sum p and m4 = sum p^2 (fp64 sums of the fp32 values
 * and of their fp64 squares); a histogram of 384 uint32 counters by an integer rule: with u = (bit pattern of p as
 * uint32) >> 20, bin = clamp(u - 696, 0, 383).  That is eight bins per octave of power from 2^-40 to 2^8; zero and
 * everything below go to bin 0, everything above to bin 383.  (p = 0, 1e-13, 2^-40, 0.09, 1, 255.9, 256, 1e9 fall into the
 * bins 0, 0, 0, 291, 320, 383, 383, 383.)  With u = b + 696 the lower edge of bin b is 2^((u >> 3) - 127) (1 + (u & 7) / 8).
 * Spectral part, of p, as the modulation monitor treats the MPX: segment j covers [j H, j H + N) and belongs to record
 * floor(j H / M); periodic Hann window, built in double and rounded once to fp32; one-sided density over k = 0 .. 512,
 * P_j[k] = c_k |sum_n w[n] p[j H + n] exp(-2 pi i k n / N)|^2 / (F sum w^2), c_k = 2 inside and 1 at both ends.  A segment
 * that holds a non-finite p is skipped and counted in segments_skipped; psd is the mean of the counted P_j (fp64 sum on
 * the device, divided on the host when read), all zeros when segments = 0.
 * Completion, ring and info as fmr_enable_monitor: record i is complete in the call that delivers the sample
 * (i + 1) M + 511; max_records = L records per stream, an overwritten unread record is counted in records_dropped; the
 * read positions live on the host.
 * Reproducibility: counts, histogram, p_min, p_max, segments and segments_skipped are bit-identical for any cut of the
 * input into calls; m2, m4 and psd add fixed per-segment values in fp64 in a fixed order without float atomics (the same
 * cut gives the same bits; another cut differs at fp64 rounding). */
#define FMR_RF_HIST_BINS 384
#define FMR_RF_PSD_BINS 513
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_rf_monitor_config) as the caller knows it (0: cfg_size); a larger size is refused */
  uint32_t interval_samples;  /* M: a multiple of 512 in 512 .. 2^30; 0 = 38400 (100 ms) */
  int max_records;            /* L: 1 .. 4096; 0 = 64 */
} fmr_rf_monitor_config;
typedef struct {
  uint64_t index, first_sample;   /* i and i M */
  uint32_t n_finite, n_nonfinite, segments, segments_skipped;
  float p_min, p_max;
  double m2, m4;
} fmr_rf_monitor_record;
typedef struct {
  unsigned struct_size;
  int hist_bins, psd_bins;        /* 384; 513 */
  uint64_t records_complete;      /* since create (of every stream: they run in step) */
  uint64_t records_dropped;       /* of this stream: overwritten unread */
  uint64_t first_unread;          /* index of the oldest unread record after this call */
  uint64_t records_ready;         /* complete records still unread after this call */
  uint32_t interval_samples;      /* M and L as enabled (defaults filled in) */
  int max_records;
  double bin_hz;                  /* F / N = 375 */
} fmr_rf_monitor_info;
/* With M2 = sum m2 / sum n_finite, M4 = sum m4 / sum n_finite (both 0 when no sample is finite) and B(lo, hi) = sum of
 * psd[k] F / N over lo <= k F / N <= hi.  0 dBFS is a full-scale complex sinusoid (|x| = 1), the scale
 * fmr_station.level_db uses.
 * C/N by second and fourth moments, for a constant-modulus carrier in complex Gaussian noise: d = 2 M2^2 - M4,
 * S = sqrt(d) when d > 0, otherwise 0, Nn = M2 - S.  The noise bandwidth is the chain's IF bandwidth (what the front end
 * passes to the decoder at 384 kHz), not a normalised one.  Any variation of the envelope -- synchronous AM, multipath --
 * reads as noise, so cn_db is a lower bound on the true C/N.
 * Envelope modulation relative to the carrier, from the spectrum of p (p ~ A^2 (1 + 2 m(t)) for small m). */
typedef struct {
  unsigned struct_size;
  int reserved;
  double level_dbfs;              /* 10 log10(M2); -INFINITY when M2 <= 0 */
  double carrier_dbfs;            /* 10 log10(S); -INFINITY when S = 0 */
  double noise_dbfs;              /* 10 log10(Nn); -INFINITY when Nn <= 0 */
  double cn_db;                   /* 10 log10(S / Nn); -INFINITY when S = 0, +INFINITY when S > 0 and Nn <= 0 */
  double am_rms;                  /* sqrt(max(M4 / M2^2 - 1, 0)) / 2: relative rms fluctuation of the envelope; 0 when M2 <= 0 */
  double am_audio_db;             /* 10 log10(B(750, 15000) / (4 M2^2)) */
  double am_pilot_db;             /* 10 log10(B(18250, 19750) / (4 M2^2)) */
  double am_floor_dbc_hz;         /* 10 log10(mean psd[k] over 100 kHz <= k F / N <= 150 kHz / (4 M2^2)); all three -INFINITY where the argument is <= 0 or M2 <= 0 */
  double p10_dbfs, p50_dbfs, p90_dbfs;   /* 10 log10 of the lower edge of the smallest bin whose cumulative count c satisfies
                                          * 100 c >= q n_finite (q = 10, 50, 90); -INFINITY when n_finite = 0 or hist is NULL */
  uint64_t n_finite, segments;    /* pooled */
} fmr_rf_monitor_levels;
/* The rules of fmr_enable_monitor: the fields are checked first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a
 * size larger than this library's struct), then the chain: NULL is FMR_ERR_BAD_ARG; any FMR_MODE_FM chain is accepted;
 * every other mode and front-end-only chains are FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's first sample: a
 * second call, or one after any processing call, is FMR_ERR_BAD_ARG.  No FM chain shape is refused: in every one of them
 * (-f, the equaliser, either resampler class, banks, the three-kernel front ends, FMR_DEBUG_TAPS=1, pipelined or in_order)
 * the decoder's input stays in the call's IF slot until that call's tail has run; no kernel of an FM chain writes the slot
 * in place.  A chain that never calls it allocates nothing for the RF monitor and runs none of its kernels. */
int fmr_enable_rf_monitor(fmr_chain *c, const fmr_rf_monitor_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap complete records of `stream`, oldest first, and returns how
 * many: recs[cap], hist[cap x 384] and psd[cap x 513] (either may be NULL).  cap = 0 returns the number waiting and drains
 * nothing.  info (may be NULL) takes info_size bytes (0 = this header's size).  FMR_ERR_BAD_ARG on a chain without the RF
 * monitor. */
int fmr_rf_monitor_read(fmr_chain *c, int stream, fmr_rf_monitor_record *recs, uint32_t *hist, double *psd, int cap,
                        fmr_rf_monitor_info *info, size_t info_size);
/* Host only, in double, no device.  Pools n records (hist: n x 384 and psd: n x 513 as read; either may be NULL): sums,
 * counts and histograms add, psd is weighted by segments; fills the levels above. */
int fmr_rf_monitor_derive(const fmr_rf_monitor_record *recs, const uint32_t *hist, const double *psd, int n,
                          fmr_rf_monitor_levels *out, size_t out_size);

/* --- Output stage: what the reference's stream loop does behind the decoder (main.cpp:950-1002),
 * on the device.  A decoder chain of any mode with it enabled delivers, per stream / bank channel, the squelched and scaled
 * audio as S16 or F32 PCM -- the bytes -R / -W and -F / -G put into the file -- and one small record per block with the
 * loop's meters (the "IF=...dB AF=...dB" pair).  The chain's double audio, fmr_status, PPS events, RDS groups and every
 * monitor's records are what they are without it: the stage only reads the finished audio and the blocks' IF RMS.
 * Everything below is per stream, runs over the blocks handed to the chain since create, in order, and does not depend
 * on how the blocks are grouped into calls.
 * Blocks and frames: `block` counts every block handed in, 0-based, empty ones included.  A block that yields no IF
 * sample leaves no record and changes no state (main.cpp:933-936).  A frame is one audio sample per channel; channels
 * is 2 for a stereo FM chain (interleaved L/R) and 1 otherwise.  first_frame is the absolute index of the block's first
 * audio frame, n_frames the number of its frames (0 for a block with IF samples that completes no audio sample).
 * if_rms: the decoder's get_if_rms() after this block, as float32 -- the very bits fmr_status.if_rms reads when a call
 * ends at this block.
 * if_level = (float)(0.75 (double)if_level + 0.25 (double)if_rms), from 0, for every block with IF samples (main.cpp:976).
 * gate_open = ((double)if_rms >= squelch_level), also for a block without audio.
 * Audio meters (main.cpp:989-996), when n_frames > 0, over the block's n = channels n_frames audio doubles before the
 * gain: each is narrowed to float32, x_f = (float)x; S1 = sum x_f and S2 = sum x_f^2 in fp64 (x_f^2 the fp64 product) in
 * a fixed order: partial t, t = 0 .. 255, adds the frames t, t + 256, ... in ascending order, channel 0 before channel 1;
 * the partials 64 w .. 64 w + 63 are joined by a butterfly (lane i adds lane i xor 32, then 16, 8, 4, 2, 1), the four
 * results added in ascending w.  audio_mean = (float)(S1 / n), audio_rms = (float)sqrt(S2 / n),
 * audio_level = (float)(0.95 (double)audio_level + 0.05 (double)audio_rms), from 0.  A block without audio repeats the
 * previous audio_level and has audio_mean = audio_rms = 0.
 * PCM: y = x g in fp64, g = gain when the gate is open and 0.0 when it is closed (adjust_gain, main.cpp:999-1002).
 *   FMR_PCM_S16: rint(y 32767.0), ties to even (AudioFileWriter's lrint(x * 32767)), saturated to [-32768, 32767]; every
 *     saturated sample counts in n_clipped (+-Inf among them); NaN becomes 0; NaN and +-Inf count in n_nonfinite.  The
 *     result differs from AudioFileWriter's only where that one overflows.
 *   FMR_PCM_F32: (float)y, non-finite values passed through and counted in n_nonfinite; n_clipped counts |y| > 1.
 * n_clipped and n_nonfinite count the values of all of the block's frames, per channel value.
 * PCM ring: max_frames interleaved frames per stream, frame f at slot f mod max_frames.  When unread frames would be
 * overwritten the oldest are dropped and counted in frames_dropped; frames that later frames of the same call overwrite
 * are never written.  Record ring: max_blocks records per stream by the same rule (blocks_dropped).  Processing never
 * fails because of either.  The read positions live on the host. */
enum { FMR_PCM_S16 = 0, FMR_PCM_F32 = 1 };
typedef struct {
  unsigned struct_size;       /* sizeof(fmr_output_config) as the caller knows it (0: cfg_size); a larger size is refused */
  int format;                 /* FMR_PCM_S16 or FMR_PCM_F32 */
  double squelch_level;       /* linear, finite, >= 0; 0 = never closed (the reference's default: if_rms >= 0) */
  double gain;                /* finite, > 0; 0 = 0.5 (-6 dB, main.cpp:1000) */
  uint32_t max_frames;        /* PCM ring per stream in frames: 1 .. 2^26; 0 = 2^18 */
  uint32_t max_blocks;        /* record ring per stream: 1 .. 65536; 0 = 4096 */
} fmr_output_config;
typedef struct {
  uint64_t block, first_frame;
  uint32_t n_frames, channels;
  float if_rms, if_level, audio_mean, audio_rms, audio_level;
  uint32_t gate_open, n_clipped, n_nonfinite;
} fmr_output_block;
typedef struct {
  unsigned struct_size;
  int format, channels;
  uint64_t first_frame;           /* absolute index of the first frame this call returned, or of the next one if none */
  uint64_t frames_waiting;        /* frames / records still unread after this call */
  uint64_t frames_dropped;        /* of this stream: overwritten unread, since create */
  uint64_t blocks_waiting, blocks_dropped;
} fmr_output_info;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field; also a size larger than this library's
 * struct), then the chain: NULL is FMR_ERR_BAD_ARG; any chain with a decoder is accepted (every mode, banks, pipelined
 * or in_order); front-end-only chains (mode -1, channelizers) are FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's
 * first block: a second call, or one after any processing call, is FMR_ERR_BAD_ARG.  A chain that never calls it
 * allocates nothing for the stage and runs none of its kernels. */
int fmr_enable_output(fmr_chain *c, const fmr_output_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap_frames frames of `stream`, oldest first, into pcm
 * (interleaved int16 or float32; *n_frames, if not NULL, takes their number) and up to cap_blocks records into blocks;
 * the two drains are independent.  Returns the number of records drained.  cap_frames = 0 and cap_blocks = 0 drain
 * nothing: info (may be NULL; info_size bytes, 0 = this header's size) says what waits.  FMR_ERR_BAD_ARG for pcm = NULL
 * with cap_frames > 0, blocks = NULL with cap_blocks > 0, a bad stream index and a chain without the stage. */
int fmr_output_read(fmr_chain *c, int stream, void *pcm, size_t cap_frames, fmr_output_block *blocks, int cap_blocks,
                    size_t *n_frames, fmr_output_info *info, size_t info_size);
/* pow(10, -(db / 20)): the linear squelch level of the reference's -l option (main.cpp:486).  Host only. */
double fmr_squelch_level_from_db(double db);

/* --- Output stage at other rates and mono: the PCM ring at rate = 48000 L / M by a polyphase
 * filter, and / or a stereo chain's frames downmixed to one channel.  The block records do not change in any field:
 * first_frame, n_frames, n_clipped, n_nonfinite and the meters keep speaking of the decoder's 48 kHz frames and of x g
 * before the filter; so do the chain's audio, fmr_status, PPS events, RDS groups and every monitor's records.
 * fmr_output_read's info.channels, first_frame, frames_waiting, frames_dropped and max_frames / cap_frames then count the
 * ring's frames, at the new rate and channel count.  The first ring frame made from a block whose first_frame is f is
 * ceil(f L / M).
 * Definition, per stream, over the audio frames since create; nothing depends on blocks or calls except the gate:
 *   x[j] is the decoder's frame j (doubles); g(j) = gain if the gate of the block holding j is open, else 0.0.
 *   z[j] = x[j] g(j) per channel; with mono on a stereo chain u = (xL + xR) 0.5 and z = u g.  z[j] = +0.0 for j < 0.
 *   Ring frame m = 0, 1, ... takes q = floor(m M / L), p = (m M) mod L and acc = 0.0; for k = 0 .. T - 1 ascending
 *   acc = acc + h[k L + p] z[q - k], every product and every sum rounded by itself in fp64 (no fused multiply-add).
 *   acc is converted by the rules of FMR_PCM_S16 / FMR_PCM_F32 above and counted in pcm_clipped / pcm_nonfinite.
 *   Frame m exists as soon as x[q] does: after F decoder frames the ring has received ceil(F L / M) frames.
 *   With L = M = 1 (mono alone) there is no filter: acc = z[j].
 * A non-finite x therefore reaches up to T ring frames (and a closed gate rings out over T frames before the ring is
 * exactly zero).
 * h is the prototype of fmr_output_rate_taps: a Kaiser-windowed sinc at rate 48000 L of T L taps, symmetric bit for bit
 * about (T L - 1) / 2, sum h = L; pass band 0 .. 0.9 rate / 2 within +-0.001 dB, stop band from rate / 2 on >= 100 dB
 * down (design attenuation 110 dB, cutoff 0.95 rate / 2). */
typedef struct {
  unsigned struct_size;   /* as the other configs: 0 = cfg_size; larger than the library's is refused */
  int rate;               /* PCM rate in Hz.  0 or 48000: the decoder's rate, no filter.  Otherwise a whole rate,
                             8000 <= rate < 48000, with L = rate / gcd(rate, 48000) <= 160 (8000, 11025, 12000, 16000,
                             22050, 24000, 32000, 44100, ...; 8001 is refused) */
  int mono;               /* 1: a stereo chain's frames become u = (xL + xR) * 0.5 before gate and filter; PCM has one
                             channel.  Ignored by chains whose audio is mono already.  Other values than 0 / 1 refused */
  int reserved;           /* must be 0 */
} fmr_output_rate_config;
/* Checks its fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field, also with a NULL chain), then the chain:
 * allowed once, after fmr_enable_output and before the chain's first block; a chain without the stage, a second call and
 * a call after any processing call are FMR_ERR_BAD_ARG.  rate 0 / 48000 with mono 0 (or with mono 1 on a chain whose
 * audio is mono) is accepted and leaves the stage exactly as it is: same kernels, same bytes.  A chain that never calls
 * it allocates nothing for the converter and runs none of its kernels. */
int fmr_set_output_rate(fmr_chain *c, const fmr_output_rate_config *cfg, size_t cfg_size);
typedef struct {
  unsigned struct_size;
  int rate, channels;            /* of the PCM ring */
  int L, M, taps_per_phase;      /* rate / 48000 = L / M in lowest terms; T (1 without a filter) */
  double delay_frames;           /* group delay in OUTPUT frames: (T L - 1) / (2 M); 0 without a filter */
  uint64_t frames_in;            /* decoder-rate frames taken since create */
  uint64_t pcm_clipped, pcm_nonfinite;   /* of this stream since create, counted on the resampled values by the rules
                                            of FMR_PCM_S16 / FMR_PCM_F32, per channel value, every produced frame.  0 on
                                            a stage left as it is (no filter, no downmix): its block records count */
} fmr_output_rate_info;
/* Synchronises like the other getters.  FMR_ERR_BAD_ARG for a bad stream, a chain without the stage, and an info_size
 * larger than this library's struct.  Valid with or without a call of fmr_set_output_rate. */
int fmr_get_output_rate(fmr_chain *c, int stream, fmr_output_rate_info *info, size_t info_size);
/* Host only, no device: the prototype filter of `rate` (T L doubles, tap i of the prototype at taps[i]) and L, M, T (each
 * may be NULL).  Returns T L, also with taps = NULL or cap too small (then nothing is written); rate 48000 (or 0) gives the
 * single tap 1.0.  FMR_ERR_BAD_ARG for a rate fmr_set_output_rate refuses. */
int fmr_output_rate_taps(int rate, double *taps, int cap, int *L, int *M, int *T);

/* --- MPX output: every stream's / bank channel's composite baseband -- the 384 kHz MPX the chain
 * demodulates on the device, which the modulation monitor measures and the RDS stage reads -- as mono PCM at
 * rate = 384000 L / M, for MPX analysers, external RDS / RDS2 decoders, archive recorders and a later stereo decode.
 * Off unless enabled; the stage only reads the MPX: the chain's audio, fmr_status, PPS events, RDS groups, every monitor's
 * records and the output stage's PCM are what they are without it.
 * Definition, per stream, over the MPX samples since the chain's first sample; nothing depends on blocks or calls:
 *   x[j] is MPX sample j as the fp32 value it is; 1.0 means 75 kHz deviation, as in the modulation monitor.
 *   z[j] = (double)x[j] gain, one fp64 product.  z[j] = +0.0 for j < 0.
 *   Ring frame m = 0, 1, ... takes q = floor(m M / L), p = (m M) mod L and acc = 0.0; for k = 0 .. T - 1 ascending
 *   acc = acc + h[k L + p] z[q - k], every product and every sum rounded by itself in fp64 (no fused multiply-add).
 *   acc is converted by the rules of FMR_PCM_S16 / FMR_PCM_F32 above (S16: rint(acc 32767), ties to even, saturated; NaN
 *   becomes 0) and counted in pcm_clipped / pcm_nonfinite as in fmr_output_rate_info.
 *   Frame m exists as soon as x[q] does: after F MPX samples the ring has received ceil(F L / M) frames.
 *   At rate 384000 there is no filter: L = M = T = 1 and acc = z[j].
 * h is the prototype of fmr_mpx_output_taps, the design rule of fmr_output_rate_taps with 384000 in place of 48000: a
 * Kaiser-windowed sinc at rate 384000 L of T L taps, symmetric bit for bit about (T L - 1) / 2, sum h = L; pass band
 * 0 .. 0.9 rate / 2 within +-0.001 dB, stop band from rate / 2 on >= 100 dB down (design attenuation 110 dB, cutoff
 * 0.95 rate / 2).  At 192000 the pass band reaches 86.4 kHz: pilot, stereo subcarrier, RDS and the RDS2 carriers.
 * PCM ring: max_frames mono frames per stream, frame f at slot f mod max_frames.  When unread frames would be overwritten
 * the oldest are dropped and counted in frames_dropped, exactly as in fmr_output_read; processing never fails because of
 * the ring.  The read positions live on the host. */
typedef struct {
  unsigned struct_size;   /* as the other configs: 0 = cfg_size; larger than the library's is refused */
  int format;             /* FMR_PCM_S16 or FMR_PCM_F32 */
  int rate;               /* PCM rate in Hz.  0 or 384000: the MPX as it is, no filter.  Otherwise a whole rate,
                             96000 <= rate < 384000, with L = rate / gcd(rate, 384000) <= 160: 96000, 171000 (3 x 57 kHz,
                             57 / 128), 192000 (1 / 2), 228000 (12 x 19 kHz, 19 / 32), 256000 (2 / 3), ...; 100001 is refused */
  double gain;            /* finite, > 0; 0 = 0.5: S16 full scale is +-150 kHz, a legal +-75 kHz station never clips */
  uint32_t max_frames;    /* PCM ring per stream in frames: 1 .. 2^26; 0 = 2^20 */
} fmr_mpx_output_config;
typedef struct {
  unsigned struct_size;
  int format, rate;
  int L, M, taps_per_phase;      /* rate / 384000 = L / M in lowest terms; T (1 without a filter) */
  double delay_frames;           /* group delay in ring frames: (T L - 1) / (2 M); 0 without a filter */
  double full_scale_hz;          /* the deviation that PCM 1.0 (S16: 32767) stands for: 75000 / gain */
  uint64_t first_frame;          /* absolute index of the first frame this call returned, or of the next one if none */
  uint64_t frames_waiting;       /* frames still unread after this call */
  uint64_t frames_dropped;       /* of this stream: overwritten unread, since create */
  uint64_t samples_in;           /* MPX samples taken since create */
  uint64_t pcm_clipped, pcm_nonfinite;   /* of this stream since create, every produced frame, by the rules of the format */
} fmr_mpx_output_info;
/* Checks the fields first (FMR_ERR_BAD_ARG, fmr_last_error names the field, also with a NULL chain; also a size larger
 * than this library's struct), then the chain: NULL is FMR_ERR_BAD_ARG; any FMR_MODE_FM chain is accepted (plain and
 * fmr_create_rds chains, banks, both resampler classes, pipelined or in_order, with the IF filter and the equaliser);
 * other modes and front-end-only chains (mode -1, channelizers) are FMR_ERR_UNSUPPORTED.  Allowed once, before the chain's
 * first sample: a second call, or one after any processing call, is FMR_ERR_BAD_ARG.  A chain that never calls it
 * allocates nothing for the stage and runs none of its kernels. */
int fmr_enable_mpx_output(fmr_chain *c, const fmr_mpx_output_config *cfg, size_t cfg_size);
/* Synchronises like the other getters, then drains up to cap_frames frames of `stream`, oldest first, into pcm (int16 or
 * float32) and returns their number (*n_frames, if not NULL, takes it too).  cap_frames = 0 drains nothing: info (may be
 * NULL; info_size bytes, 0 = this header's size) says what waits.  FMR_ERR_BAD_ARG for pcm = NULL with cap_frames > 0, a
 * bad stream index, a chain without the stage and an info_size larger than this library's struct. */
int fmr_mpx_output_read(fmr_chain *c, int stream, void *pcm, size_t cap_frames, size_t *n_frames, fmr_mpx_output_info *info,
                        size_t info_size);
/* Host only, no device: the prototype filter of `rate` (T L doubles) and L, M, T (each may be NULL), with the contract of
 * fmr_output_rate_taps.  rate 384000 (or 0) gives the single tap 1.0.  FMR_ERR_BAD_ARG for a rate fmr_enable_mpx_output
 * refuses. */
int fmr_mpx_output_taps(int rate, double *taps, int cap, int *L, int *M, int *T);

/* --- MPX input: an FM chain that is fed composite baseband -- an MPX archive written through
 * fmr_enable_mpx_output, a stereo generator's output sampled by a 192 kHz sound card, another receiver's MPX -- as mono PCM
 * at rate = 384000 L / M instead of IQ.  Its front end brings the PCM to the 384 kHz MPX; from there on it is the FM chain:
 * pilot PLL, stereo decode, audio tail, and with rds = 1 the RDS decoder of fmr_create_rds.  There is no IF: no resampler,
 * no IF AGC, no discriminator.
 * Definition, per stream, over the frames since create; nothing depends on blocks or calls:
 *   L / M = rate / 384000 in lowest terms; h is the prototype of fmr_mpx_output_taps(rate): T L taps at rate 384000 L,
 *   sum h = L.
 *   Frame i gives u[i].  FMR_PCM_S16: (double)v / 32767.0, one fp64 division.  FMR_PCM_F32: (double)v; a non-finite value
 *   becomes +0.0 and counts in nonfinite_in.
 *   z[i] = u[i] g', g' = gain ((double)M / (double)L), formed once on the host.  z[i] = +0.0 for i < 0.
 *   MPX sample j = 0, 1, ... takes i0 = floor(j L / M), p = j L - i0 M and acc = 0.0; for k = 0, 1, ... ascending while
 *   p + k M < T L: acc = acc + h[p + k M] z[i0 - k] -- at most K = ceil(T L / M) terms, every product and every sum rounded
 *   by itself in fp64 (no fused multiply-add).  x[j] = (float)acc, round to nearest even.
 *   Sample j exists as soon as u[i0] does: after F frames the chain has taken ceil(F M / L) MPX samples, and a block yields
 *   the difference of that count across it (this can be 0; such a block behaves as a block without IF samples does on an
 *   IQ chain).  Group delay: (T L - 1) / (2 L) MPX samples.
 *   At rate 384000 there is no filter: x[j] = (float)(u[j] gain).
 * x stands where the discriminator output stands on an IQ chain; 1.0 means 75 kHz deviation.  With gain 1.0 at 384000 F32
 * the chain reproduces, bit for bit, the audio, PPS events and RDS groups of the IQ chain whose fmr_enable_mpx_output ring
 * (384000, F32, gain 1.0) it is fed.
 * fmr_status: if_rms = 0, if_agc_gain = 1, agc_iterations = agc_fallback = 0, the multipath fields 0; baseband_mean /
 * baseband_level are formed as on an IQ chain (the same sums in the same order); everything else as on an FM chain.
 * fmr_debug_read: tap 1 is the MPX of the most recent call, taps 2 and 3 as on an FM chain, tap 5 as on an RDS chain when
 * rds = 1; taps 0, 4, 6 and 7 are FMR_ERR_BAD_ARG.
 * Accepted stages: fmr_enable_monitor, _loudness, _analyser, _weak_signal, _mpx_output, and _output with
 * squelch_level == 0.  FMR_ERR_UNSUPPORTED: fmr_enable_output with a squelch level (there is no IF level to gate on),
 * fmr_enable_rf_monitor, fmr_enable_blanker, fmr_enable_iq_correction.  fmr_process* and fmr_resample* on such a chain are
 * FMR_ERR_BAD_ARG, and so are fmr_process_mpx_blocks* on any other chain. */
typedef struct {
  unsigned struct_size;   /* as the other configs: 0 = in_size; larger than the library's is refused */
  int format;             /* FMR_PCM_S16 or FMR_PCM_F32 */
  int rate;               /* 0 or 384000: MPX as it is; else a rate fmr_enable_mpx_output accepts (96000 <= rate < 384000,
                             rate / gcd(rate, 384000) <= 160) */
  double gain;            /* finite, > 0; 0 = 2.0, the inverse of the MPX output's default 0.5 */
  int rds;                /* 1: with the RDS decoder, as fmr_create_rds */
} fmr_mpx_input_config;
typedef struct {
  unsigned struct_size;
  int format, rate;
  int L, M, taps_per_phase;      /* rate / 384000 = L / M in lowest terms; T (1 without a filter) */
  int taps_per_sample;           /* K = ceil(T L / M) (1 without a filter) */
  double delay_samples;          /* group delay in MPX samples: (T L - 1) / (2 L); 0 without a filter */
  double full_scale_hz;          /* the deviation that PCM 1.0 (S16: 32767) stands for: 75000 gain */
  uint64_t frames_in;            /* PCM frames taken since create */
  uint64_t samples_out;          /* MPX samples made of them: ceil(frames_in M / L) */
  uint64_t nonfinite_in;         /* of this stream since create: F32 frames that were NaN or +-Inf (taken as +0.0) */
} fmr_mpx_input_info;
/* cfg: mode = FMR_MODE_FM and enable_resampler = 0 are required; n_streams, stereo, deemphasis_us, pilot_shift,
 * max_block_len and max_blocks (in frames), device and struct_size are honoured; input_rate must be 0 or the PCM rate;
 * filter_coeff is not needed.  FMR_ERR_UNSUPPORTED for another mode, fmfilter_enable, multipath_stages > 0,
 * input_format != FMR_IQ_CF32 and enable_fourth_down; FMR_ERR_BAD_ARG for enable_resampler, channel_offset_hz, and a bad
 * format, rate or gain (fmr_last_error names the field).  Every refusal is made before the device is opened.  The chain
 * is in-order.  cfg_size / in_size: the sizes of the structs as the caller knows them, 0 = this header's. */
int fmr_create_mpx_decoder(const fmr_config *cfg, size_t cfg_size, const fmr_mpx_input_config *in, size_t in_size, fmr_chain **out);
/* pcm holds n_streams rows of stream_stride mono frames of the chain's format; block_len is in frames.  Otherwise the
 * contract of fmr_process_blocks: audio rows of audio_stride doubles, audio_len[b] the doubles block b produced, the
 * capacity checked before any state advances. */
int fmr_process_mpx_blocks(fmr_chain *c, const void *pcm, size_t stream_stride, const uint32_t *block_len, int n_blocks,
                           double *audio, size_t audio_stride, uint32_t *audio_len);
/* The contract of fmr_process_blocks_device; the device rows and their stride (in bytes) are 16-byte aligned, as for the
 * raw IQ formats. */
int fmr_process_mpx_blocks_device(fmr_chain *c, const void *d_pcm, size_t stream_stride, const uint32_t *block_len,
                                  int n_blocks, double *d_audio, size_t audio_stride, uint32_t *audio_len, int sync);
/* Synchronises like the other getters.  FMR_ERR_BAD_ARG for a bad stream, a chain that is not an MPX decoder, and an
 * info_size larger than this library's struct (0 = this header's size). */
int fmr_get_mpx_input_info(fmr_chain *c, int stream, fmr_mpx_input_info *info, size_t info_size);
/* Host only, no device: L, M, T, K and the group delay in MPX samples of `rate` (each may be NULL).  rate 384000 (or 0)
 * gives 1, 1, 1, 1 and 0.  FMR_ERR_BAD_ARG for a rate fmr_enable_mpx_output refuses. */
int fmr_mpx_input_geometry(int rate, int *L, int *M, int *T, int *K, double *delay_samples);
/* fmr_debug_chain_shape for fmr_create_mpx_decoder: what that create would decide, or its refusal.  No device. */
int fmr_debug_mpx_chain_shape(const fmr_config *cfg, size_t cfg_size, const fmr_mpx_input_config *in, size_t in_size,
                              fmr_chain_shape_info *out, size_t out_size);

#ifdef __cplusplus
}
#endif
#endif
