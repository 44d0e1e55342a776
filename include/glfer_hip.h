/* glfer_hip.h -- C-ABI of the MI355X spectral-estimation engine (libglfer_hip.so).
 *
 * This is the drop-in boundary for glfer's L2 "spectral estimator" layer: the calls
 * that source.c:141-158 makes once per hop (fft_do + fft_psd, mtm_do) and that
 * g_main.c:1109,1153-1183 makes once per drawn column (compute_floor, update_avg_*).
 * The reference has no FFI; its boundary is that C function interface, so the
 * replacement is (a) a batch API over a whole sample stream (this file) and (b)
 * signature-compatible per-hop shims built on it (glfer_compat.h).
 *
 * Plain C types only: pointers, sizes, ints, floats.  Device pointers are HIP device
 * addresses (hipMalloc / torch tensor data_ptr); `hip_stream` is a hipStream_t passed
 * as void* (NULL = the default stream).  All functions return 0 on success or a
 * negative GLFER_E_* code; glfer_hip_strerror() names it.  Nothing here falls back to
 * the CPU: without a usable HIP device every compute entry point fails with
 * GLFER_E_HIP.
 *
 * Device memory the library takes by itself: what a plan holds (tables; freed by
 * glfer_hip_plan_destroy) and per-call scratch, given back in stream order.  Scratch requests of
 * 16 MiB and more (averaged rows, a mean-corrected stream copy, big-block and LMP / F-test
 * intermediates) come from up to six blocks per device that the library keeps until the process ends
 * -- the stream-ordered allocator costs milliseconds, now and then seconds, per GB-sized request.
 * GLFER_SCRATCH_CACHE=0 in the environment takes them from the stream-ordered pool instead.
 */
#ifndef GLFER_HIP_H
#define GLFER_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* estimator: glfer.h:47  enum {MODE_NONE=-1, MODE_FFT, MODE_MTM, MODE_HPARMA, MODE_LMP} */
#define GLFER_MODE_FFT 0
#define GLFER_MODE_MTM 1
#define GLFER_MODE_HPARMA 2
#define GLFER_MODE_LMP 3

/* window ids: fft.h:67 */
#define GLFER_WIN_HANNING 0
#define GLFER_WIN_BLACKMAN 1
#define GLFER_WIN_GAUSSIAN 2
#define GLFER_WIN_WELCH 3
#define GLFER_WIN_BARTLETT 4
#define GLFER_WIN_RECTANGULAR 5
#define GLFER_WIN_HAMMING 6
#define GLFER_WIN_KAISER 7

/* sample formats of the stream: float [-1,1), or raw PCM converted on the device with
 * the rules of wav_fmt.c:104-117 (u8: (x-128)/128, s16: x/32768) */
#define GLFER_SAMPLES_F32 0
#define GLFER_SAMPLES_S16 1
#define GLFER_SAMPLES_U8 2

/* history_mode: what the first N-H samples of a frame hold (fft.c:98-108).
 * ZERO_FIRST : zeros before the first sample only (glfer.first_buffer cleared after
 *              frame 0 -- what happens with opt.autoscale on, g_main.c:1111-1120)
 * ZERO_ALWAYS: zeros in every frame (glfer.first_buffer never cleared -- what the
 *              reference does with opt.autoscale off)                              */
#define GLFER_HISTORY_ZERO_FIRST 0
#define GLFER_HISTORY_ZERO_ALWAYS 1

/* averaging modes: glfer.h:56-58 avgmode_t */
#define GLFER_AVG_SUMAVG 1
#define GLFER_AVG_PLAIN 2
#define GLFER_AVG_SUMEXTREME 3

#define GLFER_OK 0
#define GLFER_E_ARG (-1)      /* bad argument / unsupported size             */
#define GLFER_E_HIP (-2)      /* HIP runtime error (no device, launch, copy) */
#define GLFER_E_NOMEM (-3)
#define GLFER_E_NUMERIC (-4)  /* DPSS eigen-solve did not converge           */

/* Everything the reference copies from `opt` into fft_params_t / mtm_params_t at
 * change_params() time (source.c:320-325, source.c:343-350) plus the two globals the
 * estimators read directly (opt.autoscale -> sub_mean, fft.c:186; glfer.first_buffer
 * -> history_mode, fft.c:99). */
typedef struct glfer_hip_config {
  int mode;            /* GLFER_MODE_*                                                  */
  int n;               /* opt.data_block_size; power of two, 8..1048576 (HP-ARMA: 32..32768; the halfcomplex spectrum
                          output up to 32768, the F-test up to 16384, the per-column stages up to 32769 bins)  */
  float overlap;       /* opt.data_blocks_overlap, [0,1)                                */
  int window_type;     /* opt.window_type (FFT mode; MTM forces rectangular, source.c:344) */
  float limiter_a;     /* opt.limiter_a  -> fft_params_t.a        (FFT mode only acts)  */
  int enable_limiter;  /* opt.enable_limiter -> fft_params_t.limiter                    */
  int sub_mean;        /* per-hop mean removal, fft.c:86-96: 0 off; 1 (= GLFER_SUBMEAN_EXACT, what fft_init stores:
                          sub_mean = opt.autoscale) the reference's rows; GLFER_SUBMEAN_FAST (2) the opt-in below */
  int history_mode;    /* GLFER_HISTORY_*                                               */
  float mtm_w;         /* opt.mtm_w = N*W time-bandwidth product (g-l_dpss.c:295-297)   */
  int mtm_k;           /* opt.mtm_k = kmax; kmax+1 tapers are used (mtm.c:189)          */
  int sample_format;   /* GLFER_SAMPLES_*                                               */
  int device;          /* HIP device ordinal                                            */
  int hparma_t;        /* opt.hparma_t: number of equations (rows), HP-ARMA mode (source.c:373) */
  int hparma_p_e;      /* opt.hparma_p_e: number of poles (source.c:374); q_e is fixed to -1 (source.c:375) */
  int lmp_av;          /* opt.lmp_av: periodograms in the LMP estimator's ring (source.c:397, lmp.c:85) */
  int psd_pitch;       /* OURS (round 4): floats from one PSD row to the next in the DEVICE entries' d_psd; 0 = dense rows of
                          N/2+1 floats (what every caller of the reference sees: one psd_buf, source.c:317-318).  A multiple
                          of 16 floats -- 2112 for N = 4096 -- puts every row on a 64-byte boundary: dense rows of 2049 floats
                          start 4 bytes further off the cache lines each and cap every row-writing stage at 0.58-0.61 of the
                          HBM peak (profiles/r03_streaming_ceilings.txt); d_psd then holds nframes * psd_pitch floats, the
                          first N/2+1 of a row are its bins, the rest is never written.  glfer_hip_floor_device_pitched and
                          glfer_hip_display.psd_pitch read such rows; update_avg takes the pitch as its `bins` (its band is
                          minbin..maxbin).  Not with GLFER_MODE_LMP; the host / file entries keep dense rows. */
} glfer_hip_config;

/* cfg.sub_mean.  The reference sums a hop sample after sample in a float (fft.c:88-92), and on a hop with a DC level the
 * ORDER of that sum is observable in the rows (up to 6.6e-4 of a row's maximum at |mean| = rms).
 *   GLFER_SUBMEAN_EXACT  (1: what fft_init stores, sub_mean = opt.autoscale -- the DEFAULT meaning of "on" since round 4)
 *                        the reference's rows: the means are accumulated in the reference's own order (submean_seq.hip: one
 *                        lane walks a hop, 64 hops side by side: one more read of the stream, at 6.1 TB/s) and handed to the
 *                        estimator kernels as a table (periodograms -- a form of its own at the plain periodogram's
 *                        occupancy that corrects a hop's samples once, in place --, even taper counts, 5 / 7 ... tapers at
 *                        N = 4096; the other forms read a corrected copy).  To the usual 1e-5 of the oracle whatever the
 *                        input up to N = 4096; above, where the REFERENCE's own recurrence-twiddle transform is 1e-5 and
 *                        more from exact arithmetic on noise-like frames (1.2-1.6e-5 at N = 8192 and 16384), to
 *                        max(1e-5, 1.1 x the oracle's distance from exact), the device itself within 1e-6 of exact
 *                        (tests/test_gpu_round4.py).  Cost against no mean removal on 2^30-sample device-resident f32
 *                        streams: the extra read -- C1 774 against 1 125, C2 269 against 336, C3 67 against 84 M frames/s
 *                        (bench.py's "+mean" rows; against GLFER_SUBMEAN_FAST: 0.69 / 0.94 / 0.83).  Taking the means
 *                        piece by piece so that the estimator's read of a piece comes out of the Infinity Cache was built
 *                        and measured (GLFER_EXACT_PIECE_MB): launches of a few tens of microseconds cost more than the
 *                        cache saves (profiles/r04_piecewise_means.txt) -- one piece is the default.  Behind a PCIe or file
 *                        source (the host / WAV entries) the pass is hidden: it runs per chunk at 60x the link's rate.
 *   GLFER_SUBMEAN_FAST   (2, opt-in) the hop is summed inside the estimator kernels (lane partials, then across the lanes):
 *                        the more accurate sum, 0-3 % over no mean removal (C2: the two-wavefront form, 14 %) -- and not
 *                        the reference's.  Indistinguishable (<= 1e-6 of a row's maximum) while a hop's mean is small
 *                        against its rms, i.e. for AC-coupled audio; on a hop with a DC level the rows differ at the low
 *                        bins by up to ~7e-4 x |mean|/rms of the row maximum (measured at |mean| = rms: 6.6e-4 Hanning
 *                        periodogram, 7e-5 multitaper, N = 4096, 50 % overlap; tests/test_gpu_round3.py).
 * Any other non-zero value is taken as GLFER_SUBMEAN_EXACT.  The per-hop shims (glfer_compat.h) take the reference's order. */
enum { GLFER_SUBMEAN_OFF = 0, GLFER_SUBMEAN_EXACT = 1, GLFER_SUBMEAN_FAST = 2 };
/* ABI BREAK (library 0.8 -> 0.9, round 4): the two non-zero values were swapped -- 0.8 had 1 = the in-kernel sums and 2 = the
 * reference's order.  A caller built against the 0.8 header that passes 2 now gets GLFER_SUBMEAN_FAST.  GLFER_HIP_ABI counts such
 * breaks; glfer_hip_abi_version() returns the number the LIBRARY was built with, so a host can refuse a mismatch at start-up:
 *     if (glfer_hip_abi_version() != GLFER_HIP_ABI) ...                                   ("ABI version") */
#define GLFER_HIP_ABI 5
int glfer_hip_abi_version(void);

/* Cutting a stream into launches, chunks or shards.
 * (1) Cut at frame indices that are multiples of GLFER_FRAME_ALIGN and every frame's PSD is
 *     bit-identical to the one-shot run (the multitaper kernel for odd taper counts works on
 *     aligned groups of up to 32 frames).  Other cuts are still correct, to rounding.
 * (2) A piece that starts at frame f > 0 must hold, to the left of sample f*H, the N-H history
 *     ROUNDED UP TO WHOLE HOPS: ceil((N-H)/H)*H samples.  Whole hops because per-hop mean removal
 *     (cfg.sub_mean, fft.c:86-96) corrects every history sample by the mean of the hop it arrived
 *     in, so the engine reads complete hops back.  (history_mode ZERO_ALWAYS needs no history, and
 *     no kernel loads any: the gathers of that mode start at the frame's own hop -- a piece may
 *     begin at the first byte of its allocation; tests/test_gpu_round3.py.)
 *     LMP mode adds lmp_av-1 hops: the frames its ring still holds are recomputed, not carried.
 *     The device entries take the stream's VIRTUAL base (address of sample 0), so a piece is
 *     passed as  d_piece - begin*sample_size  with frame indices left global.
 * glfer_hip_frame_range() deals a stream out over `world` ranks by these rules (the arithmetic
 * of glfer_amd/shard.py): contiguous ranges, boundaries on multiples of GLFER_FRAME_ALIGN. */
#define GLFER_FRAME_ALIGN 32
void glfer_hip_frame_range(size_t total_frames, unsigned rank, unsigned world, size_t *first, size_t *count);

typedef struct glfer_hip_plan glfer_hip_plan;

/* fft_init (fft.c:168-187) / mtm_init (mtm.c:88-151) / hparma_init (hparma.c:45-71): builds the
 * window or the DPSS tapers + eigenvalues on the host (double), uploads the device tables.
 * HP-ARMA mode (BASELINE config 5): hparma_do (hparma.c:74-157) per frame -- autocorrelation,
 * the t x (p_e+1) matrix with the reference's row-0 overflow, one-sided Jacobi SVD (util.c:261-386),
 * AR spectrum; window forced rectangular, a/limiter without effect (source.c:369-372). */
int glfer_hip_plan_create(const glfer_hip_config *cfg, glfer_hip_plan **plan_out);
/* fft_close (fft.c:297-306) / mtm_close (mtm.c:242-265) */
void glfer_hip_plan_destroy(glfer_hip_plan *plan);

int glfer_hip_hop(const glfer_hip_plan *plan);      /* H = (int)(N*(1.0-overlap)), fft.c:70 */
int glfer_hip_bins(const glfer_hip_plan *plan);     /* N/2+1, source.c:317                  */
int glfer_hip_num_tapers(const glfer_hip_plan *plan);
/* whole hops in nsamples (wav_fmt.c:119 hands out whole blocks only) */
size_t glfer_hip_num_frames(const glfer_hip_plan *plan, size_t nsamples);

/* Host copies of the tables, for inspection and parity tests.
 * window: n floats (compute_window, fft.c:309-360; all ones in MTM mode).
 * tapers: [kmax+1][n] doubles, unit energy (gl_dpss, g-l_dpss.c:288-347);
 * sig   : kmax+1 doubles, lambda_k - 1 (g-l_dpss.c:342-344). */
int glfer_hip_get_window(const glfer_hip_plan *plan, float *window);
int glfer_hip_get_tapers(const glfer_hip_plan *plan, double *tapers, double *sig);

/* The same two table generators without a plan or a device (pure host code): what
 * fft_init()/mtm_init() compute before anything touches the GPU. */
int glfer_hip_make_window(int window_type, int n, float *window);
int glfer_hip_make_dpss(int n, int kmax, double nw, double *tapers, double *sig);

/* Host only, for checking the register-resident half tables of the five-taper N = 4096 multitaper kernel (n = 4096,
 * kmax = 4) against the full tables of the same plan.  half: [256][40] floats, row t = what lane t keeps (the samples
 * r(t) + 256 m, m = 0..7, r(16 j + p) = p < 8 ? 8 j + p : 240 - 8 j + p: floats 16 P + 2 m + k = taper 2 P + k of pair
 * P = 0, 1, floats 32 + m = the last taper); pairs (optional): [2][8][256][4] = { taper 2P @m, taper 2P+1 @m, the same
 * @m+1 } for sample t + 256 m of lane t; last (optional): [4][256][4] = the last taper at m = 4 q .. 4 q + 3.
 * Returns 1 if the plan's scaled float tables are exactly (anti)symmetric about the frame centre, so that a plan keeps
 * half tables (half is filled), 0 if not (the plan keeps the full tables; half is left alone), < 0 on error. */
int glfer_hip_y_half_tables(int n, int kmax, double nw, float *half, float *pairs, float *last);

/* Host only: the launch shape of that kernel's queue form (the plain single-stream launches draw their frame pairs in
 * chunks from a counter the plan owns; GLFER_Y_QUEUE=0 in the environment keeps the static stride).  *blocks: the
 * workgroups of a launch with at least that many chunks; *chunk: consecutive frame pairs per ticket. */
void glfer_hip_y_queue_shape(int *blocks, int *chunk);

/* THE hot path: frames [first_frame, first_frame+nframes) of a device-resident stream.
 *   d_stream : device pointer to sample 0 of the stream (format = cfg.sample_format)
 *   nsamples : samples in the stream (for bounds: frame f reads [f*H-(N-H), f*H+H))
 *   d_psd    : device, [nframes][N/2+1] floats, row i = frame first_frame+i
 * Equivalent to calling fft_do+fft_psd (source.c:143-144) or mtm_do (source.c:148)
 * once per hop.  Asynchronous on hip_stream.  With sub_mean the per-hop means are
 * removed inside the estimator kernels where the hop is 2, 4, 8 or 16 sixteenths of the block
 * (overlap 87.5 / 75 / 50 / 0 %; a stream's first ceil((N-H)/H) frames and the remaining
 * forms go through a device copy of the hops involved); the reference mutates the caller's
 * buffer (fft.c:93-95), the device stream is left untouched either way.
 * GLFER_MEAN_PREPASS=1 in the environment forces the copy everywhere (A/B runs). */
int glfer_hip_spectrogram_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples,
                                 size_t first_frame, size_t nframes, float *d_psd,
                                 void *hip_stream);

/* Many independent streams of one plan in one call: the same frames [first_frame, first_frame+nframes) of each.
 *   d_streams    : stream b is d_streams + b * stream_pitch samples -- exactly what glfer_hip_spectrogram_device would
 *                  be given as d_stream (the virtual-base convention and the "Cutting a stream" rules included);
 *                  every stream has nsamples samples
 *   stream_pitch : in samples of cfg.sample_format; any value, overlapping streams included.  With s16 / u8 samples it
 *                  must be even (GLFER_E_ARG otherwise): the kernel choice reads the stream's alignment (the real-input
 *                  forms fetch integer samples in aligned pairs), and it must not differ between the streams of a batch
 *   d_psd        : device, [nstreams][nframes][pitch] floats; row i of stream b at d_psd + (b * nframes + i) * pitch
 * Every row is float for float the row glfer_hip_spectrogram_device writes for that stream on the same plan.
 * nstreams == 0 or nframes == 0: GLFER_OK, nothing launched; every other argument error is the single-stream entry's.
 * Asynchronous on hip_stream.
 * FFT and MTM modes at N = 256 .. 16384 -- mean removal, RA9MB / limiter and ZERO_ALWAYS included -- run the whole batch
 * in the launches one stream takes (the estimator, hop-means and corrected-copy kernels' stream dimension: blockIdx.y), so
 * the launch count does not grow with nstreams; a batch above the device's grid y limit (65 535) is cut into chunks of that
 * many streams.  Scratch: the corrected copies and hop-means tables of all streams at once, what the single-stream entry
 * takes for a stream of nstreams times the hops.  LMP plans run the same way: the periodograms of all streams (with the
 * min(lmp_av - 1, first_frame) frames the ring still holds, recomputed per stream) go to scratch in the batch's launches and one
 * batched statistic launch set follows (glfer_hip_lmp_batch_device's kernels); the call is cut into chunks of streams whose
 * periodograms take at most half of glfer_hip_scratch_limit's cap (8 GiB by default; one stream at least), so the launch
 * count grows with the bytes, not with nstreams.  HP-ARMA plans, at every N they accept (32 .. 32768): the corrected copies of
 * the batch's mean removal as above, then ONE launch of the HP-ARMA kernel over the flat list of all nstreams x nframes frames
 * (a wavefront per frame, the frames beyond those in flight drawn from the launch's queue across stream boundaries; 2^31 - 1
 * frames a launch, more go in pieces of whole streams): 1 kernel a call, 3 with sub_mean = 1, 2 with sub_mean = 2.  (A plan
 * made under GLFER_HPARMA_WIDTH=16 -- A/B runs -- keeps the loop over the streams.)  The other modes at N outside
 * 256 .. 16384 go stream by stream inside the call, and so does an LMP or HP-ARMA chunk of one stream.  The opt-in in-launch hop-means producers and the piecewise means (GLFER_MEANS_PRODUCERS, GLFER_EXACT_PIECE_MB)
 * are never taken by this entry.
 * The moving average of many streams: glfer_hip_spectrogram_avg_batch_device and glfer_hip_avg_batch_device below; their
 * waterfalls: glfer_hip_waterfall_batch_device.
 * The harmonic F-test of many streams: glfer_hip_mtm_ftest_batch_device below.
 * Streams of unequal length: glfer_hip_spectrogram_ragged_device below; their moving average and waterfall:
 * glfer_hip_avg_ragged_device, glfer_hip_spectrogram_avg_ragged_device and glfer_hip_waterfall_ragged_device; their F-test:
 * glfer_hip_mtm_ftest_ragged_device and glfer_hip_mtm_rows_ftest_ragged_device.
 * The channels of ONE interleaved recording as the streams of a batch: glfer_hip_spectrogram_channels_device, and from host memory
 * or a WAV file glfer_hip_spectrogram_host_channels / glfer_hip_spectrogram_wav_channels ("Multi-channel recordings" below).
 * Not covered: batched host / WAV / workers entries for independent streams, the halfcomplex-spectrum output, several GPUs.  glfer_hip_floor_device takes the nstreams x nframes rows as they are. */
int glfer_hip_spectrogram_batch_device(glfer_hip_plan *plan, const void *d_streams, size_t nstreams,
                                       size_t stream_pitch, size_t nsamples, size_t first_frame,
                                       size_t nframes, float *d_psd, void *hip_stream);

/* Ragged batches: nstreams streams of one plan, each with its own length, in one call.
 *   d_samples  : device, one buffer that holds every stream, in samples of cfg.sample_format
 *   offsets,
 *   lengths    : HOST arrays [nstreams], in samples: stream b is the lengths[b] samples at d_samples + offsets[b].  Any
 *                order, gaps and overlaps allowed (the samples are only read).  With s16 / u8 samples every offsets[b] must
 *                be even (GLFER_E_ARG otherwise), for the reason the batch entry refuses an odd pitch: the kernel choice
 *                reads a stream's alignment and must not differ between the streams of a launch.  f32 offsets are free.
 *                d_samples itself may have any alignment the single-stream entry takes: each launch reads its route from
 *                the samples it is given (the raw streams, or their corrected f32 copies), as that entry does.
 *                Both arrays are consumed before the call returns.
 *   d_psd      : device, [sum of frames][pitch] floats (cfg.psd_pitch honoured).  Stream b is processed WHOLE, from its own
 *                zero history: frames_b = lengths[b] / hop rows (none for a stream shorter than a hop), packed -- its
 *                rows start at row R_b = frames_0 + ... + frames_(b-1)
 *   row_starts : HOST, optional, [nstreams + 1]: receives R_0 .. R_nstreams
 * Stream b's rows are float for float those of glfer_hip_spectrogram_device(plan, d_samples + offsets[b], lengths[b], 0,
 * frames_b, ...).  glfer_hip_ragged_frames(plan, nstreams, lengths, row_starts) returns the total row count (and the same
 * row_starts, optional) so that d_psd can be sized first; it touches no device.  It returns 0 for a NULL plan or NULL
 * lengths, SIZE_MAX if the sum overflows.
 * FFT and MTM modes at N = 256 .. 16384 -- every sub_mean value, RA9MB / limiter and ZERO_ALWAYS included -- take a number of
 * kernel launches and copies that does not depend on nstreams or on the lengths: each launch the single-stream entry makes
 * for one stream (first frames, body, frames off the frame groups, hop means, corrected copies) is made once over all
 * streams, blockIdx.y indexing a small per-stream table the call builds and uploads; more than 65 535 streams go in chunks
 * of that many.  LMP plans: the packed periodograms go to scratch through the same launch set and the ragged statistic
 * (glfer_hip_lmp_ragged_device's kernels) runs over the same row starts, in chunks of streams whose rows take at most half of
 * glfer_hip_scratch_limit's cap (one stream at least).  HP-ARMA plans at every N they accept: one launch over the flat list of
 * all streams' frames, a per-stream table (first flat frame, samples, first row, frame0, frames; streams without frames have
 * no entry) searched by bisection -- over the raw samples, or with mean removal over corrected copies made once for all
 * streams (1 kernel a call, 3 with sub_mean = 1, 2 with sub_mean = 2).  The other modes at N outside 256 .. 16384 go stream
 * by stream inside the call, and so does a call (or a chunk) of one stream.
 * GLFER_E_ARG: NULL plan; NULL offsets / lengths with nstreams > 0; NULL d_samples or d_psd while any stream has a frame; an
 * odd offset with integer samples; a stream of more than 2^31 - 1 frames; sizes that overflow size_t -- all checked before
 * anything on the device is touched; a hip_stream that is being captured into a graph (the per-stream tables are uploaded from
 * host memory that is gone when the call returns, which a captured copy would read at every replay).  nstreams == 0 or no frame at all: GLFER_OK, nothing written.
 * Limits: whole streams only (no first_frame / nframes sub-range), device-resident samples only.  The moving average and
 * the waterfall of ragged rows: glfer_hip_avg_ragged_device, glfer_hip_spectrogram_avg_ragged_device and
 * glfer_hip_waterfall_ragged_device below; the harmonic F-test and the rows-and-F pair of ragged streams:
 * glfer_hip_mtm_ftest_ragged_device and glfer_hip_mtm_rows_ftest_ragged_device.  Not built: the average taken inside the
 * estimator launch for ragged calls, host / WAV ragged entries.  Asynchronous on hip_stream. */
size_t glfer_hip_ragged_frames(const glfer_hip_plan *plan, size_t nstreams, const size_t *lengths, size_t *row_starts);
int glfer_hip_spectrogram_ragged_device(glfer_hip_plan *plan, const void *d_samples, size_t nstreams,
                                        const size_t *offsets, const size_t *lengths, float *d_psd,
                                        size_t *row_starts, void *hip_stream);

/* In LMP mode (GLFER_MODE_LMP, lmp.c:101-181) the same entry writes the detection statistic:
 * per frame the rectangular-window periodogram of the assembled frame (lmp.c:114-125), then per
 * bin mean and variance over the ring of the last lmp_av periodograms (zeros before the stream,
 * slot order as lmp.c:134-149) and the clamped statistic of lmp.c:151-160. */

/* The statistic alone, over rectangular-window periodogram rows the caller already holds on the device (rows of an FFT plan
 * with GLFER_WINDOW rectangular and the LMP plan's n / overlap / sub_mean / history_mode, from any of the spectrogram entries:
 * an LMP plan computes exactly those rows before its statistic).  Dense rows of `bins` floats.
 *   d_rows    : frames row_first, row_first + 1, ... of one stream
 *   d_out     : [nframes][bins], the statistic of frames [first_frame, first_frame + nframes)
 * The sums run over the ring's slots in slot order and a frame's slot is frame mod lmp_av, so the frames' absolute indices are
 * arguments; the ring is empty before frame 0 and holds the last lmp_av frames: the rows must reach back
 * min(lmp_av - 1, first_frame) frames (row_first <= first_frame - that), GLFER_E_ARG otherwise.  Every output is bit for bit
 * what glfer_hip_spectrogram_device writes on the LMP plan for those frames.
 * glfer_hip_lmp_batch_device: the same over nstreams streams that share row_first, first_frame and nframes; stream b's rows at
 * d_rows + b * row_stride floats, its outputs at d_out + b * out_stride floats (strides at least a stream's rows / outputs),
 * each stream's ring empty before its frame 0.  One launch per 65 535 streams (per 65 535 groups of 16 frames), the kernels'
 * blockIdx.z the stream; ring sizes 2, 3, 4, 8 keep the ring in registers, the others up to 64 in LDS (from 64 frames a
 * stream), the rest go frame by frame.
 * glfer_hip_lmp_ragged_device: packed rows of streams of unequal length as glfer_hip_spectrogram_ragged_device writes them,
 * stream b rows [row_starts[b], row_starts[b + 1]) of d_rows and of d_out (HOST array [nstreams + 1], non-decreasing, at most
 * 2^31 - 1 rows a stream), every stream whole from its frame 0.  One launch over a flat list of frame groups (a per-stream
 * table the call builds and uploads; a stream without rows has no entry), whatever nstreams is.
 * Arguments, in this order: GLFER_E_ARG for lmp_av outside 1 .. 4096 or bins < 1; GLFER_OK with nothing launched for no
 * stream or no frame; GLFER_E_ARG for NULL row_starts or ones that decrease or hold a stream of more than 2^31 - 1 rows, for
 * NULL d_rows / d_out, rows that do not reach back far enough, strides shorter than a stream, nframes > 0x7fffffff, sizes that
 * overflow size_t; the ragged entry refuses a hip_stream that is being captured (its table is uploaded from host memory).
 * Asynchronous on hip_stream. */
int glfer_hip_lmp_device(const float *d_rows, size_t row_first, size_t first_frame, size_t nframes, int bins, int lmp_av,
                         float *d_out, void *hip_stream);
int glfer_hip_lmp_batch_device(const float *d_rows, size_t nstreams, size_t row_stride, size_t row_first, size_t first_frame,
                               size_t nframes, int bins, int lmp_av, float *d_out, size_t out_stride, void *hip_stream);
int glfer_hip_lmp_ragged_device(const float *d_rows, size_t nstreams, const size_t *row_starts, int bins, int lmp_av,
                                float *d_out, void *hip_stream);

/* Same, also writing the halfcomplex spectrum of each tapered frame in the layout of
 * fft_radix2.c:75-177 (data[k]=Re X_k, data[N-k]=Im X_k).  FFT mode only: this is
 * what fft_do leaves in params->outbuf.  d_spec: [nframes][N] floats. */
int glfer_hip_spectrum_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples,
                              size_t first_frame, size_t nframes, float *d_psd, float *d_spec,
                              void *hip_stream);

/* prepare_audio (fft.c:66-165) on its own: what it leaves in params->inbuf_fft for every frame
 * (history, RA9MB, window, limiter) -- lmp.c:101-120 and the scope (g_scope.c:194-197) read it.
 * d_frames: [nframes][N] floats. */
int glfer_hip_prepare_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples,
                             size_t first_frame, size_t nframes, float *d_frames, void *hip_stream);

/* The harmonic F-test that mtm_do computes beside the spectrum (mtm.c:165-174 mu = transform of
 * the hn-windowed frame; mtm.c:203-210 denominator; mtm.c:222-233 F = k |mu|^2 sum(U0^2) / den).
 * MTM plans only.  d_ftest: [nframes][N/2+1] floats.
 *   mu_live = 0: the reference as built without FFTW -- the transform at mtm.c:173 runs in place
 *                and `mu` stays zero, so F is 0 (NaN where the denominator is 0);
 *   mu_live = 1: mu as the FFTW build computes it (mtm.c:171) -- the statistic as intended.
 * Quirks kept: the Nyquist bin's denominator is never accumulated (x/0), its numerator counts
 * mu[N/2] twice; sums in float with double terms, as the reference's declarations give. */
int glfer_hip_mtm_ftest_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples,
                               size_t first_frame, size_t nframes, float *d_ftest, int mu_live,
                               void *hip_stream);

/* glfer_hip_mtm_ftest_device for nstreams streams laid out as glfer_hip_spectrogram_batch_device takes them: stream b is
 * d_streams + b * stream_pitch samples, nsamples long, starting with zero history -- what the single entry would be given
 * as d_stream -- and the same frames [first_frame, first_frame + nframes) of each.
 *   d_ftest : device, [nstreams][nframes][N/2+1] floats; row i of stream b at d_ftest + (b * nframes + i) * (N/2+1), dense
 *             whatever cfg.psd_pitch is, as in the single entry
 * Every row is bit for bit the row glfer_hip_mtm_ftest_device writes for that stream on the same plan (the Nyquist column's
 * x/0 included), with the same mu_live.  Asynchronous on hip_stream.
 * Arguments, in this order: GLFER_E_ARG for a NULL plan; for a plan that is not MTM or has N > 16384; then GLFER_OK with
 * nothing launched for nstreams == 0 or nframes == 0; then GLFER_E_ARG for a NULL d_streams or d_ftest, a frame past the
 * stream, nframes > 0x7fffffff, an odd stream_pitch with s16 / u8 samples (the reason given at
 * glfer_hip_spectrogram_batch_device: every stream of a batch must meet the same kernels), or sizes that overflow size_t.
 * N = 256 .. 16384 run the whole batch in the launches one stream takes: the F statistic's kernel carries the stream as
 * blockIdx.y, in both of its forms (one sequence per transform, and two separated through the mirror bins; the form is chosen
 * as the single entry chooses it, GLFER_FTEST_PAIRED read per call, paired from N = 2048 by default), and mean removal
 * (sub_mean 1 and 2) goes through the batch's corrected copies and hop-means tables, so the launch count does not grow with
 * nstreams.  A batch above the device's grid y limit (65 535) is cut into chunks of that many streams.  Scratch under mean
 * removal: the corrected float copies of all streams' hops at once.  N < 256 (the spectra go through memory and a per-bin
 * epilogue forms the statistic) goes stream by stream inside the call, the single entry's launches per stream.
 * The F-test tables are made by the first F call on a plan, whichever entry it is; the plan is left as the single entry leaves it.
 * The multitaper rows and F from one pass over the samples: glfer_hip_mtm_rows_ftest_device and its batch form below.
 * Streams of unequal length (one length per stream): glfer_hip_mtm_ftest_ragged_device below.
 * Not built: batched host / WAV entries. */
int glfer_hip_mtm_ftest_batch_device(glfer_hip_plan *plan, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                     size_t nsamples, size_t first_frame, size_t nframes, float *d_ftest, int mu_live,
                                     void *hip_stream);

/* The two things mtm_do computes from the same tapered transforms of a frame (mtm.c:154-239) in one call and one pass over
 * the samples: the weighted eigenspectrum sum (mtm.c:212-219: the rows glfer_hip_spectrogram_device writes for an MTM plan)
 * and the harmonic F statistic (glfer_hip_mtm_ftest_device).  Every sample is read once, mean removal runs once and every
 * taper's transform is computed once; a caller who wants one of the two has the entries above.
 *   d_psd   : device, [nframes][cfg.psd_pitch or N/2+1] floats, laid out as glfer_hip_spectrogram_device lays its rows out;
 *             the floats between N/2+1 and the pitch are not touched
 *   d_ftest : device, [nframes][N/2+1] floats, dense, as in glfer_hip_mtm_ftest_device
 * Both are required.  MTM plans only, N <= 16384.
 * The F rows are bit for bit glfer_hip_mtm_ftest_device's for the same call (same mu_live, same GLFER_FTEST_PAIRED).  The PSD
 * rows are sum_j |y_j|^2 / (N (1 + sig_j)) taken from the F transforms -- each taper's own real-input spectrum, summed in float
 * in taper order -- so they agree with glfer_hip_spectrogram_device's rows to float rounding, not bit for bit (that entry packs
 * two tapers per transform with the weights folded into its tables).
 * N = 256 .. 16384: one launch; each taper's round of the F kernel also adds its weighted |y_j|^2 to a per-bin sum in
 * registers, in both forms of that kernel.  N < 256: the spectra go through memory as for F, and the per-bin epilogue forms
 * the rows from them too.  Mean removal, history_mode and frame ranges as in the F entry.
 * The batch form takes the streams as glfer_hip_mtm_ftest_batch_device does (stream b at d_streams + b * stream_pitch, zero
 * history); stream b's PSD rows start at d_psd + (b * nframes) * pitch, its F rows at d_ftest + (b * nframes) * (N/2+1), and
 * both hold the bits of the single entry for that stream.  N >= 256: the launches of one stream (blockIdx.y is the stream;
 * chunks of the grid's y limit); N < 256: stream by stream.
 * Arguments (both entries; the single one as a batch of one stream), in this order: GLFER_E_ARG for a NULL plan; for a plan
 * that is not MTM or has N > 16384; then GLFER_OK with nothing launched for nstreams == 0 or nframes == 0; then GLFER_E_ARG
 * for a NULL d_stream(s), d_psd or d_ftest, a frame past the stream, nframes > 0x7fffffff, an odd stream_pitch with s16 / u8
 * samples (batch), or sizes that overflow size_t.
 * The F-test tables are made by the first F call on a plan, whichever entry it is; the plan is left as the F entry leaves it. */
int glfer_hip_mtm_rows_ftest_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples, size_t first_frame,
                                    size_t nframes, float *d_psd, float *d_ftest, int mu_live, void *hip_stream);
int glfer_hip_mtm_rows_ftest_batch_device(glfer_hip_plan *plan, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                          size_t nsamples, size_t first_frame, size_t nframes, float *d_psd, float *d_ftest,
                                          int mu_live, void *hip_stream);

/* The F entries for streams of unequal length in one call: glfer_hip_mtm_ftest_device and glfer_hip_mtm_rows_ftest_device over
 * the streams glfer_hip_spectrogram_ragged_device takes.  d_samples, offsets, lengths and row_starts mean exactly what they mean
 * there: one device buffer, HOST offsets / lengths in samples consumed before the call returns, any order, gaps and overlaps
 * free, even offsets with s16 / u8 samples; row_starts (HOST, optional, [nstreams + 1]) receives R_0 .. R_nstreams.
 * Each stream is processed WHOLE, from its own zero history: stream b yields frames_b = lengths[b] / hop rows, packed from row
 * R_b = frames_0 + ... + frames_(b-1) on; glfer_hip_ragged_frames sizes both outputs.
 *   d_ftest : device, [sum of frames][N/2+1] floats, dense whatever cfg.psd_pitch is, as in every F entry
 *   d_psd   : device (rows-and-F), [sum of frames][cfg.psd_pitch or N/2+1] floats; the floats between N/2+1 and the pitch are
 *             not touched
 * Stream b's F rows are bit for bit those glfer_hip_mtm_ftest_device(plan, d_samples + offsets[b], lengths[b], 0, frames_b, ...)
 * writes, and its F and PSD rows from the rows-and-F entry those of glfer_hip_mtm_rows_ftest_device for the same arguments --
 * same mu_live, same GLFER_FTEST_PAIRED, the Nyquist column's x/0 included.  history_mode ZERO_FIRST and ZERO_ALWAYS both.
 * Arguments, in this order (1-8 before any device is touched):
 *   1. GLFER_E_ARG for a NULL plan;
 *   2. GLFER_E_ARG for a plan that is not MTM or has N > 16384;
 *   3. GLFER_OK with row_starts[0] = 0 and nothing launched for nstreams == 0;
 *   4. GLFER_E_ARG for NULL offsets / lengths;
 *   5. GLFER_E_ARG for any of the ragged rows entry's per-stream checks: more than 2^31 - 1 frames in a stream, an odd offset
 *      with integer samples, sizes that overflow size_t (rows sized with the pitch for the rows-and-F entry, with N/2+1 for F);
 *   6. row_starts is filled;
 *   7. GLFER_OK with nothing written if no stream has a frame;
 *   8. GLFER_E_ARG for a NULL d_samples, d_ftest or (rows-and-F) d_psd;
 *   9. GLFER_E_ARG for a hip_stream under graph capture (the per-stream tables are uploaded from host memory that is gone when
 *      the call returns, as in glfer_hip_spectrogram_ragged_device).
 * N = 256 .. 16384 with two or more streams: a launch count that depends neither on nstreams nor on the lengths.  With sub_mean
 * 1 or 2, one set of hop-means and corrected-copy launches over hops [0, frames_b) of every stream (the F entries correct every
 * frame through copies, so there is no head / body / tail cut), then ONE launch of the F statistic's kernel; without mean
 * removal that one launch from the raw samples.  blockIdx.y indexes a per-stream table that carries the stream's samples, its
 * first PSD row (in units of the pitch) and, separately, its first F row (in units of N/2+1).  The form -- one sequence per
 * transform or paired -- is chosen as the single entry chooses it.  More than 65 535 streams go in chunks of that many; a chunk
 * of one stream, a call of one stream and N < 256 go through the single entry, stream by stream inside the call.
 * The F-test tables are made once per call at most; the plan is left as the single entry leaves it.  Asynchronous on hip_stream.
 * Not built: sub-ranges of a ragged stream, host / WAV ragged F entries. */
int glfer_hip_mtm_ftest_ragged_device(glfer_hip_plan *plan, const void *d_samples, size_t nstreams, const size_t *offsets,
                                      const size_t *lengths, float *d_ftest, int mu_live, size_t *row_starts, void *hip_stream);
int glfer_hip_mtm_rows_ftest_ragged_device(glfer_hip_plan *plan, const void *d_samples, size_t nstreams, const size_t *offsets,
                                           const size_t *lengths, float *d_psd, float *d_ftest, int mu_live, size_t *row_starts,
                                           void *hip_stream);

/* Host-buffer entry: h_stream goes to the device in chunks through a two-deep ring (two pinned
 * sample buffers, two device buffers each way; uploads on one stream, kernels and downloads on two:
 * a chunk goes up while the previous chunk's rows come down), the PSD rows come back; blocks until done.
 * h_psd in pinned memory (glfer_hip_host_alloc) receives its rows by DMA directly, and an h_stream
 * in pinned memory is uploaded from where it lies; any other memory goes through pinned staging
 * and a host copy (the slower way by 3-4x: the host copy sets the pace).
 * *nframes_out receives glfer_hip_num_frames(nsamples). */
int glfer_hip_spectrogram_host(glfer_hip_plan *plan, const void *h_stream, size_t nsamples,
                               float *h_psd, size_t *nframes_out);

/* Pinned host memory for the ring's ends (source.c / wav_fmt.c side buffers). */
/* (pinned with the calling thread on the CPUs of the current device's NUMA node, its affinity restored afterwards;
 * GLFER_NUMA_BIND=0 turns the placement off) */
void *glfer_hip_host_alloc(size_t bytes);
void glfer_hip_host_free(void *p);

/* The same over several GPUs of one node: the frame range is dealt out with
 * glfer_hip_frame_range() over the devices whose bit is set in device_mask (bit d = HIP device
 * d; cfg->device is ignored), one host thread per GPU, each with its own plan, streams and
 * pinned ring; every GPU reads its hops plus the history rule (2) above from h_stream and writes
 * a disjoint row range of h_psd.  No data moves between GPUs (frames are independent:
 * source.c:130-158 is a loop over hops).  Rows are bit-identical to the one-GPU run. */
int glfer_hip_spectrogram_host_multi(const glfer_hip_config *cfg, unsigned device_mask,
                                     const void *h_stream, size_t nsamples, float *h_psd,
                                     size_t *nframes_out);
/* Host-side placement: every worker thread of the *_multi / *_workers entries is bound, before it makes its
 * plan and pinned ring, to the CPUs of its GPU's NUMA node -- /sys/bus/pci/devices/<bus id>/numa_node and
 * /sys/devices/system/node/node<N>/cpulist, intersected with the CPUs this process may use -- so pinned staging memory,
 * and the first touch of the worker's range of the caller's rows, land beside the GPU; the calling thread's own
 * affinity is restored.  Unknown node (-1), a one-worker call or GLFER_NUMA_BIND=0: nothing is bound.  The two
 * look-ups are exported (sysfs_root NULL = "/sys"): the node of a PCI bus id (-1 = unknown) and a node's CPUs as a bit
 * mask (returns how many, -1 on a missing or malformed list). */
int glfer_hip_numa_node_of_bus_id(const char *bus_id, const char *sysfs_root);
int glfer_hip_numa_node_cpus(int node, const char *sysfs_root, unsigned char *mask, size_t mask_bytes);

/* The same with the workers listed: one host thread + plan + streams + pinned ring per entry of
 * devices[0..nworkers); an ordinal may repeat (workers then share that GPU -- how a one-GPU machine
 * runs, and tests, the multi-worker path).  _multi is this with the mask's devices, one worker each. */
int glfer_hip_spectrogram_host_workers(const glfer_hip_config *cfg, const int *devices, int nworkers,
                                       const void *h_stream, size_t nsamples, float *h_psd,
                                       size_t *nframes_out);

/* ---- ingest: the file source of source.c:118-128 / wav_fmt.c:45-121 ------------------------
 * The canonical 44-byte RIFF/WAVE header of wav_fmt.h:34-52, read with fixed-width fields
 * (the reference's struct uses u_long and mis-parses every file on LP64 hosts).  As in the
 * reference only PCM (format 1) with 8 or 16 bits per sample is accepted and the channel
 * count is not interpreted by glfer_hip_spectrogram_wav and its _ex / _range / _multi / _workers forms: interleaved channels are
 * treated as one sample stream (wav_fmt.c ignores `modus`).  glfer_hip_spectrogram_wav_channels reads `channels` and gives every
 * channel its own rows ("Multi-channel recordings" below).  The RIFF
 * chunks are walked ("fmt ", then "data"; "LIST" / "fact" / ... skipped), so a file with other
 * chunks before or after its samples is read correctly -- the reference's fixed 44-byte struct
 * (wav_fmt.h:34-52) would play them as samples; a file that cannot be walked is read its way. */
typedef struct glfer_wav_info {
  int format;            /* 1 = PCM                                  wav_fmt.h:42 */
  int channels;          /* "modus": 1 mono, 2 stereo                wav_fmt.h:43; read by glfer_hip_spectrogram_wav_channels only */
  int sample_rate;       /* sample_fq                                wav_fmt.h:44 */
  int bits_per_sample;   /* bit_p_spl: 8 or 16                       wav_fmt.h:47 */
  size_t data_offset;    /* first byte of the "data" chunk's payload (44 in the reference's fixed layout) */
  size_t nsamples;       /* samples in the data chunk                             */
  size_t data_bytes;     /* bytes in the data chunk (to the end of the file when the chunk size is 0 / ~0 / too long) */
} glfer_wav_info;
int glfer_hip_wav_probe(const char *path, glfer_wav_info *info);

/* Whole-file spectrogram: reads `path` hop block by hop block through two pinned host
 * buffers (the next block is read from the file while the GPU works on the current one),
 * uploads the raw PCM with hipMemcpyAsync -- the conversion of wav_fmt.c:104-117 happens in
 * the kernel's gather -- and writes frame rows to h_psd ([max_frames][N/2+1], host).
 * plan->sample_format must match the file (8 bit: GLFER_SAMPLES_U8, 16 bit: _S16).
 * chunk_frames = frames per upload (0 = default 16384). */
int glfer_hip_spectrogram_wav(glfer_hip_plan *plan, const char *path, float *h_psd, size_t max_frames,
                              size_t *nframes_out, size_t chunk_frames);
/* flags = GLFER_WAV_PARTIAL_TAIL: a file whose data is not a whole number of hop blocks yields
 * one more frame, as in the reference: wav_read (wav_fmt.c:102-119) converts the samples of the
 * short last read over the STALE rest of its buffer -- the previous block as the estimator left it
 * (prepare_audio removes the hop's mean in place, fft.c:93-95) -- and reports a block.  An odd last
 * byte of a 16-bit file is dropped (n_read/2 samples).  Without the flag (and in
 * glfer_hip_spectrogram_wav) whole blocks only.  Not available in LMP mode. */
#define GLFER_WAV_PARTIAL_TAIL 1u
int glfer_hip_spectrogram_wav_ex(glfer_hip_plan *plan, const char *path, float *h_psd, size_t max_frames,
                                 size_t *nframes_out, size_t chunk_frames, unsigned flags);

/* The same for frames [first_frame, first_frame + max_frames) of the file only: rows to h_psd[0 ..).
 * (The per-hop shims' read-ahead walks a file in such windows, glfer_compat.h.) */
int glfer_hip_spectrogram_wav_range(glfer_hip_plan *plan, const char *path, size_t first_frame, size_t max_frames,
                                    float *h_psd, size_t *nframes_out, size_t chunk_frames, unsigned flags);

/* ---- Multi-channel recordings: every interleaved channel as its own stream -----------------------------------------------------
 * A recording of C channels holds sample frames: sample i of channel c is element i * C + c.  Every entry above reads such a
 * buffer or file as ONE stream L R L R ... (the reference's behaviour, and still theirs); the entries here take the channel count
 * and give each selected channel the rows the single-stream entries give on a contiguous copy of it.
 * In all of them: channels is 1 .. 64; select is a HOST array of nselect (1 .. 64) channel indices, each < channels, duplicates
 * allowed, consumed before the call returns; select == NULL means all channels in order (nselect is then ignored and the number
 * selected is `channels`).  channels == 1 with select == NULL calls the single-stream entry directly: no copy is made.
 *
 * glfer_hip_deinterleave_device: the kernel alone (channels.hip), for callers who feed the other batch entries themselves (the
 * F-test, the averages, the waterfall, rows-and-F):  d_out[j * out_pitch + i] = d_in[i * channels + select[j]]  for i < nframes
 * sample frames.  Samples are moved as bytes, never converted.  out_pitch, in samples, must be >= nframes; d_in and d_out may
 * have any alignment the sample size allows and must not overlap.  ONE launch, no table upload: legal on a hip_stream that is
 * being captured.  Stereo (channels == 2) runs a form with 16-byte loads and 8-byte stores per lane over the longest run for which
 * d_in and every plane written are aligned for it (chosen on the host from the pointers and the pitch: the source on whole sample
 * frames from a 16-byte boundary, the planes 8-byte aligned there), and a lane-per-sample-frame form over the rest; every other
 * channel count runs the latter.  GLFER_CHANNELS_WIDE=0 in the environment keeps the general form everywhere (A/B runs).
 * Arguments, in this order, nothing on the device touched before they pass: GLFER_E_ARG for channels outside 1 .. 64, nselect
 * outside 1 .. 64 with a non-NULL select or an index >= channels; for an unknown sample_format; for out_pitch < nframes; then
 * GLFER_OK with nothing launched for nframes == 0; then GLFER_E_ARG for a NULL d_in or d_out, or sizes that overflow size_t.
 * Asynchronous on hip_stream. */
int glfer_hip_deinterleave_device(const void *d_in, size_t nframes, int channels, int sample_format, const int *select, int nselect,
                                  void *d_out, size_t out_pitch, void *hip_stream);

/* Frames [first_frame, first_frame + nframes) of every selected channel of a device-resident interleaved recording.
 *   d_samples            : sample frame 0 of the recording (format = cfg.sample_format), under the virtual-base convention of
 *                          the other device entries ("Cutting a stream": a piece is passed as d_piece - begin * channels *
 *                          sample_size with the frame indices left global)
 *   nsamples_per_channel : sample frames in the recording
 *   d_psd                : device, [nselect][nframes][pitch] floats (cfg.psd_pitch honoured); row i of selection j at
 *                          d_psd + (j * nframes + i) * pitch
 * The rows of selection j are float for float the rows glfer_hip_spectrogram_device writes for the same frames of a contiguous
 * copy of channel select[j] in the same sample format -- for every plan glfer_hip_spectrogram_batch_device takes (FFT, MTM and LMP
 * at every N, HP-ARMA at every N it accepts), every sub_mean value, both history modes, f32 / s16 / u8.
 * Only the hops those frames read are de-interleaved -- their own and the left halo of "Cutting a stream", ceil((N-H)/H) hops plus
 * lmp_av - 1 for an LMP plan, none below hop 0 -- into stream-ordered scratch planes, each starting 16-byte aligned, a multiple
 * of 16 bytes apart; the body of glfer_hip_spectrogram_batch_device then runs on the planes' virtual base with the frame indices
 * left global: its kernels plus one.  Planes of more than half of glfer_hip_scratch_limit's cap: the call is cut into pieces of
 * frames that end on GLOBAL multiples of GLFER_FRAME_ALIGN (at least GLFER_FRAME_ALIGN frames each while the call has that many
 * left), each with its own halo, so the rows do not depend on the cut (glfer_amd/csrc/channel_cuts.h).
 * Arguments, in this order, nothing on the device touched before they pass: GLFER_E_ARG for a NULL plan; for channels outside
 * 1 .. 64, nselect outside 1 .. 64 with a non-NULL select or an index >= channels; then GLFER_OK with nothing launched for
 * nframes == 0; then GLFER_E_ARG for a NULL d_samples or d_psd, a frame past the recording, nframes > 0x7fffffff, sizes that
 * overflow size_t.  Asynchronous on hip_stream. */
int glfer_hip_spectrogram_channels_device(glfer_hip_plan *plan, const void *d_samples, size_t nsamples_per_channel, int channels,
                                          const int *select, int nselect, size_t first_frame, size_t nframes, float *d_psd,
                                          void *hip_stream);

/* The same from host memory and from a WAV file, through the chunk ring of glfer_hip_spectrogram_host in ONE pass over the data:
 * a chunk of whole hops of sample frames is read and uploaded interleaved (a hop is hop * channels * sample_size bytes for the
 * reader, the chunk's 256 MiB cap, the halo kept from the previous chunk and the upload), de-interleaved on the device into a
 * second device buffer of the ring, run as a batch of the selected channels and downloaded plane by plane.  Blocking.
 *   h_psd        : host, [nselect][F][N/2+1] floats, plane j the rows of channel select[j]; F = the frame count for the host
 *                  entry (glfer_hip_num_frames(nsamples_per_channel)), max_frames for the file entry -- the caller's allocation,
 *                  so it must be a real size when more than one channel is selected
 *   *nframes_out : frames per channel: for a file (its size in whole sample frames) / hop, clipped to max_frames; a trailing
 *                  incomplete sample frame or hop is dropped
 * The file's channel count comes from its header.  Plane j equals glfer_hip_spectrogram_host's rows on the extracted channel.
 * Limits: rows only (no waterfall), one plan on one GPU, whole hops only (GLFER_WAV_PARTIAL_TAIL is defined for one stream), dense
 * rows (a plan with cfg.psd_pitch is refused, as by every host entry).
 * Arguments, in this order, nothing on the device touched before they pass: GLFER_E_ARG for a NULL plan (path, nframes_out); [file:
 * the probe's error for a file that is no PCM WAV, GLFER_E_ARG for a bit depth that does not match the plan;] GLFER_E_ARG for
 * channels outside 1 .. 64, nselect outside 1 .. 64 with a non-NULL select or an index >= channels; for a pitched plan; then
 * GLFER_OK with *nframes_out = 0 for a recording shorter than a hop; then GLFER_E_ARG for NULL buffers or sizes that overflow
 * size_t. */
int glfer_hip_spectrogram_host_channels(glfer_hip_plan *plan, const void *h_samples, size_t nsamples_per_channel, int channels,
                                        const int *select, int nselect, float *h_psd, size_t *nframes_out);
int glfer_hip_spectrogram_wav_channels(glfer_hip_plan *plan, const char *path, const int *select, int nselect, float *h_psd,
                                       size_t max_frames, size_t *nframes_out, size_t chunk_frames);

/* ---- Complex I/Q input: two-sided rows -----------------------------------------------------------------------------------------
 * A complex-baseband recording (an SDR receiver's stereo WAV or raw buffer, I in one channel and Q in the other) holds complex
 * samples z[n] = I[n] + i Q[n], interleaved I, Q, I, Q, ... in cfg.sample_format: f32 pairs, s16 pairs (x / 32768), u8 pairs
 * ((x - 128) / 128) -- the conversions of wav_fmt.c:104-117 on each part.  Its spectrum is two-sided, N bins per frame, and is not
 * the pair of one-sided spectra the channel entries above give for I and Q.  With a plan in GLFER_MODE_FFT or GLFER_MODE_MTM:
 *   frame f            : complex samples [f H - (N - H), f H + H), H = glfer_hip_hop(plan); the history modes mean what they mean
 *                        for real streams (ZERO_FIRST: zeros before sample 0; ZERO_ALWAYS: zeros in the first N - H positions of
 *                        every frame); nsamples / H frames; the virtual-base convention and frame ranges of
 *                        glfer_hip_spectrogram_device ("Cutting a stream", in complex samples)
 *   Z_j[k]             = sum_n w_j[n] z_f[n] exp(-2 pi i k n / N),  k = 0 .. N-1
 *   periodogram        : P[k] = |Z[k]|^2 / N, w the plan's window (fft.c:212-216 over all N bins; rectangular: no window, as there)
 *   multitaper         : P[k] = sum_j |Z_j[k]|^2 / (N (1 + sig_j)) over the plan's kmax + 1 tapers (mtm.c:212-219)
 * With Q = 0 bins 0 .. N/2 are the real entry's row to rounding; a tone exp(+2 pi i k0 n / N) lands in bin k0 alone.
 * One kernel per call (spectro16c.hip; a batch above the grid's y limit: one per chunk of streams), no host synchronisation, no
 * allocation: legal on a hip_stream that is being captured.  The table [taper][N] of w_j with the scale folded in is made with
 * the plan; glfer_hip_iq_tables gives the same floats without a device.
 *   flags : GLFER_IQ_CENTERED  bin k is stored at column (k + N/2) mod N: negative frequencies left of the carrier, as a waterfall
 *                              shows it
 *           GLFER_IQ_SWAP      the first value of each pair is Q (the usual cure for a mirrored spectrum): the rows of the stream
 *                              with the two values exchanged in memory, float for float
 *   nsamples, stream_pitch : complex samples
 *   row_pitch : floats from one row to the next; 0 means N, any other value must be >= N.  cfg.psd_pitch is NOT read here
 *   d_psd     : [nframes][row_pitch]; a batch: row i of stream b at d_psd + (b * nframes + i) * row_pitch
 *   d_iq (and d_iq + b * stream_pitch) must be aligned to one complex sample: 8, 4 or 2 bytes
 * Supported (glfer_hip_iq_supported, host only: GLFER_OK or GLFER_E_ARG): FFT or MTM mode, N = 256 .. 16384, every window, every
 * taper count the plan accepts, every overlap, both history modes, the three sample formats; sub_mean must be 0 and the limiter
 * off (limiter_a <= 0, enable_limiter == 0).
 * Arguments, nothing on the device touched before they pass: GLFER_E_ARG for a NULL plan or one that is not supported, unknown
 * flag bits, a row_pitch below N; then GLFER_OK with nothing launched for nframes == 0 (nstreams == 0); then GLFER_E_ARG for NULL
 * buffers, a misaligned d_iq (stream_pitch counts complex samples, so every stream of a batch is then aligned), first_frame +
 * nframes wrapping or reaching past the stream, nframes > 0x7fffffff, sizes that overflow size_t.  Asynchronous on hip_stream.
 * Downstream: glfer_hip_floor_device, the glfer_hip_avg_* entries and the waterfall entries take a `bins` argument and work up to
 * 32769 bins, so they take these rows (bins = N <= 16384, pitch = row_pitch) as they are.
 * Not built: mean removal and the limiter / RA9MB on I/Q, N outside 256 .. 16384, ragged / host / WAV / workers / multi-GPU forms,
 * the F-test, LMP and HP-ARMA on complex input. */
#define GLFER_IQ_CENTERED 1u
#define GLFER_IQ_SWAP     2u
int glfer_hip_iq_supported(const glfer_hip_config *cfg);
/* table: host, [taper count][cfg->n] floats, w_j[n] sqrt(1 / N) (periodogram) or v_j[n] sqrt(1 / (N (1 + sig_j))), the product taken in
 * double and rounded once; NULL: the count alone.  Returns the taper count (1 for the periodogram), or a negative GLFER_E_*. */
int glfer_hip_iq_tables(const glfer_hip_config *cfg, float *table);
int glfer_hip_spectrogram_iq_device(glfer_hip_plan *plan, const void *d_iq, size_t nsamples, size_t first_frame, size_t nframes,
                                    float *d_psd, size_t row_pitch, unsigned flags, void *hip_stream);
int glfer_hip_spectrogram_iq_batch_device(glfer_hip_plan *plan, const void *d_iq, size_t nstreams, size_t stream_pitch,
                                          size_t nsamples, size_t first_frame, size_t nframes, float *d_psd, size_t row_pitch,
                                          unsigned flags, void *hip_stream);

/* ---- Two channels: multitaper cross-spectrum and coherence in one pass ---------------------------------------------------------
 * How two receivers relate, bin by bin (two antennas, a loop and a noise probe, the halves of a diversity set-up).  The input is
 * real samples of two channels, interleaved x[0], y[0], x[1], y[1], ... in cfg.sample_format: the memory layout the I/Q entries
 * read, and a stereo WAV's.  The plan is GLFER_MODE_MTM with kmax >= 1; frames, hop, history modes, the virtual base and frame
 * ranges are those of glfer_hip_spectrogram_iq_device, counted in sample pairs.  With X_j = FFT(v_j x_f), Y_j = FFT(v_j y_f) over
 * the plan's kmax + 1 tapers and c_j = 1 / (N (1 + sig_j)), for k = 0 .. N/2:
 *   Sxx[k] = sum_j c_j |X_j[k]|^2           the real entry's multitaper row of channel x, to rounding
 *   Syy[k] = sum_j c_j |Y_j[k]|^2
 *   Sxy[k] = sum_j c_j X_j[k] conj(Y_j[k])  complex; y lagging x by d samples gives angle(Sxy[k]) = +2 pi k d / N
 *   coh[k] = |Sxy[k]|^2 / (Sxx[k] Syy[k])   the magnitude-squared coherence: clamped to [0, 1], and exactly 0 where Sxx[k] Syy[k]
 *                                           is 0 (silence gives zero rows, never NaN); the quotient is formed in double, so
 *                                           spectra anywhere in float range neither underflow the product nor overflow the square
 * Im Sxy is exactly 0 at k = 0 and k = N/2.  Thomson's K tapers are what makes coh an estimate from a single frame: with one
 * window it is identically 1, so GLFER_MODE_FFT plans and kmax = 0 are refused.
 * Outputs, any subset (NULL: not wanted, not computed for the store; all four NULL is refused), P = N/2 + 1 bins a row:
 *   d_sxx, d_syy, d_coh : [nframes][row_pitch] floats; row_pitch 0 means P, any other value must be >= P
 *   d_sxy               : [nframes][sxy_pitch] float pairs (re, im), complex64's layout; sxy_pitch counts pairs, 0 means P
 *   a batch             : row i of stream b at + (b * nframes + i) rows of each output; stream b's pair 0 at d_xy + b * stream_pitch
 *                         pairs; d_xy must be aligned to one pair (8, 4 or 2 bytes)
 * One kernel per call (spectro16cx.hip: one packed transform per taper carries both channels, which are taken apart through the
 * mirror bins; a batch above the grid's y limit: one per chunk of streams), no allocation, no host synchronisation: legal on a
 * hip_stream that is being captured.  cfg.psd_pitch is NOT read here.
 * ACCURACY: both channels ride one transform, so a channel's separated spectrum carries the rounding of the PAIR, not its own.  If
 * one channel is tens of dB louder, the weaker one's Sxx floor sits at the louder one's rounding level (some 2^-24 of the louder
 * amplitude per bin) -- the effect README.md records for hn in the paired F-test.  Bring the channels to like level first.
 * Supported (glfer_hip_cross_supported, host only: GLFER_OK or GLFER_E_ARG): MTM mode, kmax >= 1, N = 256 .. 8192, every overlap,
 * both history modes, the three sample formats; sub_mean must be 0, the limiter and RA9MB off.
 * Arguments, nothing on the device touched before they pass: GLFER_E_ARG for a NULL plan or one that is not supported, a pitch
 * below P; then GLFER_OK with nothing launched for nframes == 0 (nstreams == 0); then GLFER_E_ARG for a NULL d_xy or all four
 * outputs NULL, a misaligned d_xy, first_frame + nframes wrapping or reaching past the stream, nframes > 0x7fffffff, sizes that
 * overflow size_t.  Asynchronous on hip_stream.
 * Not built: N = 16384 (its 1024 lanes a frame leave 128 registers a lane: the twiddles, the transform and the 36 sums do not
 * fit without spilling), a phase row (atan2 of d_sxy gives it), two
 * separate plane pointers, mean removal, ragged / host / WAV / workers forms, more than two channels (pairs of a C-channel
 * recording).  Averaging over frames, which is what gives FFT plans a coherence: the Welch entries below. */
int glfer_hip_cross_supported(const glfer_hip_config *cfg);
int glfer_hip_mtm_cross_device(glfer_hip_plan *plan, const void *d_xy, size_t nsamples, size_t first_frame, size_t nframes,
                               float *d_sxx, float *d_syy, float *d_coh, size_t row_pitch, void *d_sxy, size_t sxy_pitch,
                               void *hip_stream);
int glfer_hip_mtm_cross_batch_device(glfer_hip_plan *plan, const void *d_xy, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                     size_t first_frame, size_t nframes, float *d_sxx, float *d_syy, float *d_coh, size_t row_pitch,
                                     void *d_sxy, size_t sxy_pitch, void *hip_stream);

/* ---- Two channels, Welch's form: the cross-spectrum and coherence of L averaged segments in one pass ------------------------------
 * The estimate known as csd / coherence: X conj(Y), |X|^2 and |Y|^2 averaged over L consecutive frames, then the quotient.  It is
 * what gives a plan of ONE window a coherence at all, so GLFER_MODE_FFT plans with any of the eight windows are taken here, and
 * it is the form that carries a weak line common to two receivers over a long stretch of time.  Input, frames (hop H, N - H pairs
 * of history, both history modes), outputs, pitches and batches are those of glfer_hip_mtm_cross_device.  With J the plan's
 * tapers (1 for an FFT plan: the table is the plan's window, c = 1 / N; a rectangular window is all ones), L = segments and
 * step the frames from one output row to the next, row r averages the frames f = first_frame + r step + s, s = 0 .. L-1:
 *   Sxx[r][k] = (1/L) sum_s sum_j c_j |X_{f,j}[k]|^2          Syy likewise
 *   Sxy[r][k] = (1/L) sum_s sum_j c_j X_{f,j}[k] conj(Y_{f,j}[k])
 *   coh[r][k] = |Sxy|^2 / (Sxx Syy)     in double from the unscaled sums, clamped to [0, 1], exactly 0 where Sxx Syy = 0
 * step = L is Welch's block average, step < L overlapping rows (a moving estimate), step > L skips frames.  A stream of F frames
 * has glfer_hip_welch_rows = (F - first_frame - L) / step + 1 rows, none if F - first_frame < L.  The sums run in a fixed order,
 * segments outermost in increasing s and the tapers inside, in float: a row is a function of its own frames alone, whatever the
 * range, step or batch that computes it.  They are stored times 0.25 / L rounded once to float, so segments = 1 stores the bits
 * of glfer_hip_mtm_cross_device.  A channel that holds no non-zero sample in ANY of a row's L segments gets exact zeros in its
 * spectrum, in Sxy and in coh; Im Sxy is exactly 0 at k = 0 and k = N/2.  The accuracy note above holds for every segment.
 * One kernel per call (spectro16cx.hip: the running sums stay in registers across a row's segments; a batch above the grid's y
 * limit: one per chunk of streams), no allocation, no host synchronisation: legal on a hip_stream that is being captured.
 * Supported (glfer_hip_welch_cross_supported, host only: GLFER_OK or GLFER_E_ARG): FFT and MTM plans that glfer_hip_iq_supported
 * takes, N = 256 .. 8192; 1 <= segments <= 4096 with segments * J >= 2 (one window and one segment: identically 1, refused);
 * step >= 1 and, where a block handles FPB = 4096 / N > 1 rows, (FPB - 1) step H + N <= (2^31 - 1) / (bytes of a pair): the
 * rows of a block read through one buffer descriptor.
 * Arguments: as glfer_hip_mtm_cross_device, nrows in the place of nframes -- GLFER_E_ARG for a NULL plan or an unsupported plan,
 * segments or step, a pitch below P; then GLFER_OK with nothing launched for nrows == 0 (nstreams == 0); then GLFER_E_ARG for a
 * NULL d_xy or all four outputs NULL, a misaligned d_xy, nrows above glfer_hip_welch_rows (a frame past the stream, or
 * first_frame + segments wrapping), nrows > 0x7fffffff, sizes that overflow size_t.  Asynchronous on hip_stream.
 * Not built: N = 16384, mean removal, ragged / host / WAV / workers forms, exponential (running) averaging across calls, more
 * than two channels, a phase row. */
int glfer_hip_welch_cross_supported(const glfer_hip_config *cfg, size_t segments, size_t step);
size_t glfer_hip_welch_rows(glfer_hip_plan *plan, size_t nsamples, size_t first_frame, size_t segments, size_t step);
int glfer_hip_welch_cross_device(glfer_hip_plan *plan, const void *d_xy, size_t nsamples, size_t first_frame, size_t segments,
                                 size_t step, size_t nrows, float *d_sxx, float *d_syy, float *d_coh, size_t row_pitch, void *d_sxy,
                                 size_t sxy_pitch, void *hip_stream);
int glfer_hip_welch_cross_batch_device(glfer_hip_plan *plan, const void *d_xy, size_t nstreams, size_t stream_pitch, size_t nsamples,
                                       size_t first_frame, size_t segments, size_t step, size_t nrows, float *d_sxx, float *d_syy,
                                       float *d_coh, size_t row_pitch, void *d_sxy, size_t sxy_pitch, void *hip_stream);

/* ---- Adaptive multitaper weights: leakage-resistant rows and their degrees of freedom in one pass ------------------------------
 * The multitaper row of glfer_hip_spectrogram_device is the reference's fixed-weight sum, as leaky as its leakiest taper: beside a
 * strong carrier the last taper's sidelobes, not the data, set the floor.  Thomson's adaptive weighting (1982, section V; Percival
 * & Walden eq. 368a / 370a) gives every bin its own weights: where the spectrum lies far below the frame's power the leaky
 * high-order tapers are weighted down to nothing, where it is flat all K tapers count.  Input: one real channel as
 * glfer_hip_spectrogram_device takes it (cfg.sample_format, both history modes, the virtual base, frame ranges).  With
 * K = kmax + 1, v_j the plan's unit-energy tapers, x_f the N values the transform sees (zeroed history INCLUDED), for k = 0 .. N/2:
 *   E_j[k] = |FFT(v_j x_f)[k]|^2 / N         the eigenspectra; there is NO 1 / (1 + sig_j) in them
 *   sigma2 = sum_n x_f[n]^2 / N              the frame's power
 *   beta_j = max(-sig_j, 0) formed in double and rounded to float; lambda_j = 1 - beta_j likewise (glfer_hip_adaptive_weights
 *            returns the floats the kernel gets); B_j = beta_j sigma2 / N bounds taper j's broadband leakage
 *   S      = (E_0 + E_1) / 2, then exactly `iters` sweeps of
 *              u_j = (lambda_0 S + B_0) / (lambda_j S + B_j)    u_0 = 1; a quotient whose denominator is 0 counts as 1
 *              w_j = lambda_j u_j^2
 *              S   = sum_j w_j E_j / sum_j w_j
 *   d_psd  = S after the last sweep.  It is a weighted MEAN of the eigenspectra; the row of glfer_hip_spectrogram_device is a
 *            weighted SUM, about K times larger on a flat spectrum.
 *   d_dof  = 2 (sum_j w_j)^2 / sum_j w_j^2 from the weights that formed the last sweep: between 2 and 2 K, what a detector
 *            needs to set a threshold.
 * w_j is the textbook d_j^2 = lambda_j S^2 / (lambda_j S + B_j)^2 with the factor common to all j cancelled, so u_j <= 1 and
 * sum w >= lambda_0: nothing underflows to 0 / 0 and silence gives exact zero rows and a finite dof, never NaN.
 * THE RESULT IS DEFINED BY THE SWEEP COUNT, NOT BY CONVERGENCE, and deliberately so.  After 8 sweeps every bin of a noise frame
 * is within 0.06 dB of the iteration's limit and all but a few tens of bins of a frame with a strong carrier within 0.1 dB, but
 * on the carrier's skirts the fixed-point equation has 3 - 5 roots and a handful of bins need 35 - 200 sweeps; an accelerated
 * iteration lands on another root.  All sums run in the fixed order j = 0, 1, ...: a row is a function of its own frame alone,
 * and sweep m's bits do not depend on how many sweeps follow.
 * Outputs, any subset (NULL: not wanted; both NULL is refused): [nframes][row_pitch] floats, row_pitch 0 means P = N/2 + 1, any
 * other value must be >= P; a batch: row i of stream b at + (b * nframes + i) rows, stream b's sample 0 at d_stream + b *
 * stream_pitch samples.  cfg.psd_pitch is NOT read here.
 * One kernel per call (spectro16a.hip: tapers 2r and 2r + 1 of a frame ride one packed transform and are taken apart through the
 * mirror bins; the K eigenspectra of a lane's bins stay in its registers until the frame's last taper, then the sweeps run
 * there; a batch above the grid's y limit: one per chunk of streams), no allocation, no host synchronisation: legal on a
 * hip_stream that is being captured.  ACCURACY: two tapers ride one transform, so an eigenspectrum carries the rounding of its
 * PAIR (some 2^-24 of the frame's amplitude per bin) -- far below the leakage the weighting removes.
 * Supported (glfer_hip_adaptive_supported, host only: GLFER_OK or GLFER_E_ARG): MTM mode, 1 <= kmax <= 7 (K = 2 .. 8),
 * N = 256 .. 4096, every overlap, both history modes, the three sample formats; sub_mean must be 0, the limiter and RA9MB off.
 * A plan whose lambda_j are not non-increasing in j is refused by the entries and by glfer_hip_adaptive_weights.
 * glfer_hip_adaptive_weights (host only): the K floats lambda_j and beta_j (either pointer may be NULL); returns K, or
 * GLFER_E_ARG / GLFER_E_NUMERIC.
 * Arguments, nothing on the device touched before they pass: GLFER_E_ARG for a NULL plan or one that is not supported, a pitch
 * below P, iters outside 1 .. 64; then GLFER_OK with nothing launched for nframes == 0 (nstreams == 0); then GLFER_E_ARG for a
 * NULL d_stream or both outputs NULL, a misaligned d_stream, first_frame + nframes wrapping or reaching past the stream,
 * nframes > 0x7fffffff, sizes that overflow size_t.  Asynchronous on hip_stream.
 * Not built: mean removal, N = 8192 (its instantiations spill ten registers) and N = 16384, more than 8 tapers (the
 * eigenspectra of 16 would take 144 registers a lane), ragged / host / WAV / workers forms, adaptive weights on I/Q or
 * cross-spectra, sweeps to a tolerance.  (Jackknife intervals: the section after this one.) */
int glfer_hip_adaptive_supported(const glfer_hip_config *cfg);
int glfer_hip_adaptive_weights(const glfer_hip_config *cfg, float *lambda_out, float *beta_out);
int glfer_hip_mtm_adaptive_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples, size_t first_frame, size_t nframes,
                                  float *d_psd, float *d_dof, size_t row_pitch, int iters, void *hip_stream);
int glfer_hip_mtm_adaptive_batch_device(glfer_hip_plan *plan, const void *d_stream, size_t nstreams, size_t stream_pitch,
                                        size_t nsamples, size_t first_frame, size_t nframes, float *d_psd, float *d_dof,
                                        size_t row_pitch, int iters, void *hip_stream);

/* ---- Jackknife confidence intervals for multitaper rows, in the same pass ---------------------------------------------------------
 * Whether a bump of 2 dB is real needs an interval.  The one derived from d_dof (a chi-square with dof degrees of freedom) assumes
 * Gaussian, locally white data, which is what fails on a carrier's skirts and on keyed signals; the delete-one jackknife over
 * tapers in the log domain (Thomson & Chave 1991; Percival & Walden section 7) does not.  The same kernel as the adaptive entries,
 * one launch: after a frame's last taper the lane that holds a bin's K eigenspectra and ran its sweeps also forms the statistic.
 * For a frame and a bin, with E_j the eigenspectra above, j = 0 .. K-1, w_j the final weights and S = sum w_j E_j / sum w_j:
 *   S_(i)  = sum_{j != i} w_j E_j / sum_{j != i} w_j      i = 0 .. K-1   (weights held fixed; K-1 non-negative terms summed in
 *                                                                         the order j = 0, 1, ..., skipping i)
 *   l_i    = ln( S_(i) / S )
 *   lbar   = (1/K) sum_i l_i
 *   logvar = ((K-1)/K) sum_i (l_i - lbar)^2                the jackknife variance of ln S
 * S_(i) is never formed as total - term: with one dominant taper that loses every bit.  The logarithm is taken of the ratio to S,
 * which lies near 1, and not of S_(i) itself: rows 200 dB down then do not carry |ln S| ulps into differences of a few 1e-3;
 * centring removes the reference point in exact arithmetic.
 * Degenerate cases, decided in the kernel: S == 0 (a silent frame) gives logvar = 0; S > 0 with some S_(i) == 0 (or a ratio
 * S_(i) / S that leaves the float range) gives logvar = +inf, the interval is unbounded; no logvar value is ever NaN.  For K = 2,
 * S_(i) is the other eigenspectrum, so logvar = 1/4 (ln E_1 - ln E_0)^2.
 * The weights, by `iters`:
 *   iters = 1 .. 64   the adaptive weights of the last sweep, the ones d_dof is computed from; d_psd and d_dof are then the bits
 *                     of glfer_hip_mtm_adaptive_device at the same iters.
 *   iters = 0         no sweeps, w_j = lambda_j: the eigenvalue-weighted mean (Percival & Walden 369a), intervals at close to the
 *                     fixed-weight row's cost.  d_psd = sum lambda_j E_j / sum lambda_j, d_dof = 2 (sum lambda)^2 / sum lambda^2.
 *                     (The adaptive entries above keep refusing iters = 0.)
 * THE INTERVAL at level p is  d_psd * exp(-/+ t sqrt(logvar)),  t = Student's quantile t_{K-1}((1 + p) / 2), which
 * glfer_hip_jackknife_factor returns (host only; 0 < level < 1; the closed-form distribution function for 1 .. 7 degrees of
 * freedom inverted by bisection; GLFER_E_ARG for a NULL pointer, a plan that is not supported, a level outside (0, 1)).
 * THERE IS NO BIAS CORRECTION: the interval is centred on ln d_psd, not on the jackknife's bias-corrected estimate
 * K ln S - (K-1) (ln S + lbar).  On independent unit-exponential eigenspectra with equal weights the interval at 0.95 covers the
 * true level in 0.94 of draws (K = 5 and K = 8; tests/test_jackknife_criterion.py).
 * Outputs, any subset of the three (NULL: not wanted; all three NULL is refused), rows and pitch as the adaptive entries'; one
 * launch a call (a batch above the grid's y limit: one per chunk of streams), no allocation, no host synchronisation: legal on a
 * hip_stream that is being captured.
 * Supported (glfer_hip_jackknife_supported, host only): what glfer_hip_adaptive_supported takes, at the sizes whose jackknife
 * instantiations are built -- all of them, N = 256 .. 4096 (profiles/jackknife_kernel_resources.txt).
 * Arguments: the adaptive entries' checks in their order, with iters outside 0 .. 64 refused.
 * Not built: the jackknife of coherence and of the cross-spectrum's phase (the cross kernel has no room for per-taper values at two
 * wavefronts per SIMD), bias correction, N >= 8192, ragged / host / WAV / workers forms, mean removal, intervals for the
 * fixed-weight row's 1 / (1 + sig_j) sum. */
int glfer_hip_jackknife_supported(const glfer_hip_config *cfg);
int glfer_hip_jackknife_factor(const glfer_hip_config *cfg, double level, double *t_out);
int glfer_hip_mtm_jackknife_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples, size_t first_frame, size_t nframes,
                                   float *d_psd, float *d_dof, float *d_logvar, size_t row_pitch, int iters, void *hip_stream);
int glfer_hip_mtm_jackknife_batch_device(glfer_hip_plan *plan, const void *d_stream, size_t nstreams, size_t stream_pitch,
                                         size_t nsamples, size_t first_frame, size_t nframes, float *d_psd, float *d_dof,
                                         float *d_logvar, size_t row_pitch, int iters, void *hip_stream);

/* ---- Zoom: a digital down-converter, and the two-sided rows of its output -------------------------------------------------------
 * A few tens of hertz around one carrier of a 48 kHz recording: instead of a block of a million samples whose transform covers the
 * whole band, the band is moved to 0 Hz, low-passed and decimated by D (a frequency-translating FIR, "DDC"), and the I/Q rows above
 * run at fs / D: D = 64 with N = 16384 has the resolution of N = 1048576, in rows of N bins that every per-column stage takes.
 * Definition (ddc.hip; tests/_ddc_exact.py is its float64 restatement):
 *   x[n]    the input, real or complex (interleaved I/Q as above), f32 / s16 (x / 32768) / u8 ((x - 128) / 128); x[n] = 0 for n < 0
 *   W       = round(freq 2^64) mod 2^64, freq in cycles per input sample, [-0.5, 0.5); phi(n) = (W n mod 2^64) / 2^64 turns, in
 *           64-bit integers: no drift at any stream length.  glfer_hip_ddc_phase_word(freq) returns W
 *   g[t]    = h[t] exp(+2 pi i phi(t)), t = 0 .. T-1, h the real float32 taps; the product in double, each part rounded once
 *   y[m]    = exp(-2 pi i phi(n0)) sum_t g[t] x[n0 - t],  n0 = (m + 1) D - 1,  m = 0 .. nsamples / D - 1
 *           = sum_t h[t] (x e^(-2 pi i phi))[n0 - t]: a tone at +freq goes to 0 Hz; one rotation per output, none per input sample
 * Outputs are complex64, interleaved float pairs: what glfer_hip_spectrogram_iq_device reads with an f32 plan.  The bits of y[m] do
 * not depend on the launch, range, tile or batch that computes it: the sum runs over t in an order t and D alone fix.
 * Host only, no device touched:
 *   glfer_hip_ddc_design     a Kaiser-windowed sinc low-pass in double, h[t] = 2 c sinc(2 c (t - (T-1)/2)) kaiser_beta(t), exactly
 *                            symmetric, normalised to unit sum, rounded to float.  Defaults where an argument is <= 0: ntaps =
 *                            min(8 decim + 1, 8192) -- 1 for decim = 1: the single tap 1.0, a pure mixer --, cutoff c = 0.4 / decim
 *                            (cycles per input sample), beta = 8.  Returns the tap count (taps NULL: the count alone)
 *                            or GLFER_E_ARG (decim outside 1 .. 1024, ntaps > 8192, cutoff > 0.5)
 *   glfer_hip_ddc_supported  GLFER_OK or GLFER_E_ARG: decim 1 .. 1024 and ntaps 1 .. 8192 in any combination, freq in [-0.5, 0.5),
 *                            the three sample formats, complex_in 0 or 1
 *   glfer_hip_ddc_tables     g[T][2] floats as defined above
 * The handle: glfer_hip_ddc_create uploads g once (the rotation needs no table: the negated 64-bit phase goes through one double
 * sincospi per output, each part rounded once to float); calls through it upload and allocate nothing and are legal on a stream
 * under graph capture.  One handle, one device (cfg.device).
 *   glfer_hip_ddc_device        outputs [first_out, first_out + nout) to d_out[0 .. nout).  d_in is the address of sample 0 by the
 *                               virtual-base convention of "Cutting a stream"; only samples [max(0, first_out D - (T-1)),
 *                               (first_out + nout) D) are read.  The batch of one
 *   glfer_hip_ddc_batch_device  stream b at d_in + b * stream_pitch (input samples; complex samples for complex input), its outputs
 *                               at d_out + b * out_pitch (complex samples; 0 means nout, else >= nout).  One launch (the stream is
 *                               the grid's y; more than 65535 streams: one launch per chunk of that many)
 *   glfer_hip_spectrogram_zoom_device
 *                               rows [first_frame, first_frame + nframes) of the I/Q entry over the DDC's output, a stream of
 *                               nsamples / D complex samples: the DDC outputs [first_frame H - (N - H) clipped at 0,
 *                               (first_frame + nframes) H) go to stream-ordered scratch, the I/Q kernel runs on that scratch's
 *                               virtual base.  Two kernels a call; rows bit for bit those of glfer_hip_spectrogram_iq_device over
 *                               glfer_hip_ddc_device's output.  The plan: one glfer_hip_iq_supported accepts, f32 sample format (the
 *                               baseband is f32; the handle's format is the recording's), on the handle's device.  flags:
 *                               GLFER_IQ_CENTERED only.  It takes scratch, so a hip_stream that is being captured is REFUSED
 *                               (GLFER_E_ARG); capture glfer_hip_ddc_device and the I/Q entry with a buffer of the caller's instead.
 *                               More than 2^31 - 1 DDC outputs in one call: GLFER_E_ARG (cut the frame range)
 * Arguments, in this order, nothing on the device touched before they pass: GLFER_E_ARG for a NULL handle (zoom: a NULL or
 * unsupported plan, unknown flags), an out_pitch (row_pitch) below nout (N); then GLFER_OK with nothing launched for nout == 0,
 * nstreams == 0 (nframes == 0); then GLFER_E_ARG for NULL buffers, first_out + nout wrapping or past nsamples / D (a frame past the
 * baseband), nout (nframes) > 0x7fffffff, a d_in not aligned to one input sample (one complex sample for complex input), sizes that
 * overflow.  Asynchronous on hip_stream.
 * Not built: ragged / host / WAV / workers / multi-GPU forms, zoom batches, swapped I/Q input, rational resampling, a fused
 * DDC-plus-transform kernel. */
typedef struct glfer_hip_ddc_config {
  int decim;           /* D: 1 .. 1024                                                        */
  int ntaps;           /* T: 1 .. 8192                                                        */
  double freq;         /* cycles per input sample, [-0.5, 0.5): what is moved to 0 Hz         */
  int complex_in;      /* 0: real samples; 1: interleaved I/Q pairs                           */
  int sample_format;   /* GLFER_SAMPLES_*                                                     */
  int device;          /* HIP device ordinal                                                  */
} glfer_hip_ddc_config;
typedef struct glfer_hip_ddc glfer_hip_ddc;
unsigned long long glfer_hip_ddc_phase_word(double freq);
int glfer_hip_ddc_design(int decim, int ntaps, double cutoff, double beta, float *taps);
int glfer_hip_ddc_supported(const glfer_hip_ddc_config *cfg);
int glfer_hip_ddc_tables(const glfer_hip_ddc_config *cfg, const float *taps, float *g);
int glfer_hip_ddc_create(const glfer_hip_ddc_config *cfg, const float *taps, glfer_hip_ddc **ddc);
void glfer_hip_ddc_destroy(glfer_hip_ddc *ddc);
int glfer_hip_ddc_device(glfer_hip_ddc *ddc, const void *d_in, size_t nsamples, size_t first_out, size_t nout, void *d_out,
                         void *hip_stream);
int glfer_hip_ddc_batch_device(glfer_hip_ddc *ddc, const void *d_in, size_t nstreams, size_t stream_pitch, size_t nsamples,
                               size_t first_out, size_t nout, void *d_out, size_t out_pitch, void *hip_stream);
int glfer_hip_spectrogram_zoom_device(glfer_hip_plan *plan, glfer_hip_ddc *ddc, const void *d_in, size_t nsamples, size_t first_frame,
                                      size_t nframes, float *d_psd, size_t row_pitch, unsigned flags, void *hip_stream);

/* BASELINE config 4 as worded ("1-hour 48 kHz WAV, frame-batch sharded across 8 x MI355X"): the
 * file's frames dealt out over the GPUs named in device_mask (glfer_hip_frame_range: contiguous
 * ranges, boundaries on multiples of GLFER_FRAME_ALIGN), one host thread + plan + pinned ring per
 * GPU, every worker reading its own part of the file -- its hops and the history halo in front of
 * them -- through its own handle (source.c:193, wav_fmt.c:45-121); rows land in disjoint ranges of
 * h_psd [frames][N/2+1]; no collective.  _workers: the workers listed; an ordinal may repeat (several
 * workers then share that GPU -- how a one-GPU box exercises the path).  cfg->sample_format must
 * match the file; flags as glfer_hip_spectrogram_wav_ex (the partial block belongs to the last worker). */
int glfer_hip_spectrogram_wav_multi(const glfer_hip_config *cfg, unsigned device_mask, const char *path, float *h_psd,
                                    size_t max_frames, size_t *nframes_out, unsigned flags);
int glfer_hip_spectrogram_wav_workers(const glfer_hip_config *cfg, const int *devices, int nworkers, const char *path,
                                      float *h_psd, size_t max_frames, size_t *nframes_out, unsigned flags);

/* ---- a persistent set of workers for the *_workers / *_multi entries (round 5) -------------------------------------------------
 * The stateless entries above make everything a worker needs inside the call.  For BASELINE config 4 as worded -- a 1-hour WAV,
 * 346 MB, 10 546 frames, 1.2 ms of kernels -- that set-up WAS the call: DPSS tapers (0.1-0.3 s at N = 16384, kept by the library
 * after the first plan), tables uploaded per plan, 30-40 ms of pinned and device buffers per worker unless the device's one parked
 * ring was free.  A handle keeps, per worker: its plan (tables on its GPU) and ITS OWN chunk ring, sized at creation for jobs of
 * hint_frames frames in all (0 = the default chunk); calls through the handle allocate nothing.  One call at a time per handle
 * (a second one waits).  The stateless entries keep the two most recently used handles themselves (same configuration and worker
 * list -> same handle; GLFER_SCRATCH_CACHE=0 or glfer_hip_scratch_limit(0): nothing is kept, glfer_hip_scratch_trim(device, 0)
 * drops them), so repeated calls are fast there too -- what a handle adds is the set-up OUTSIDE the first call.
 * phases (may be NULL): where the call's time went -- per field the largest value over the workers (they run side by side),
 * seconds: set-up inside the call (ring look-up, any allocation), reading / copying the samples into pinned memory, uploads,
 * kernels (from a chunk's upload end to its kernels' end), downloads -- sums over a worker's chunks, which OVERLAP one another, so
 * the fields add up to more than wall_s -- and the call's wall time; chunks = chunks of all workers. */
typedef struct glfer_hip_phases {
  double setup_s, read_s, h2d_s, kernel_s, d2h_s, wall_s;
  unsigned chunks;
} glfer_hip_phases;
typedef struct glfer_hip_workers glfer_hip_workers;
int glfer_hip_workers_create(const glfer_hip_config *cfg, const int *devices, int nworkers, size_t hint_frames,
                             glfer_hip_workers **out);
void glfer_hip_workers_destroy(glfer_hip_workers *w);
/* glfer_hip_spectrogram_wav_workers / glfer_hip_spectrogram_host_workers through a handle */
int glfer_hip_workers_spectrogram_wav(glfer_hip_workers *w, const char *path, float *h_psd, size_t max_frames,
                                      size_t *nframes_out, unsigned flags, glfer_hip_phases *phases);
int glfer_hip_workers_spectrogram_host(glfer_hip_workers *w, const void *h_stream, size_t nsamples, float *h_psd,
                                       size_t *nframes_out, glfer_hip_phases *phases);

/* K0 on its own: per-hop mean removal (fft.c:86-96).  d_out[i] = sample(d_in[i]) - mean of the
 * hop i belongs to; nhops hops of `hop` samples each.  (The spectrogram entries apply it
 * themselves when cfg.sub_mean is set; this entry serves the per-hop shims, which must hand
 * the corrected hop back to the caller as the reference does.) */
int glfer_hip_submean_device(const void *d_in, float *d_out, int hop, size_t nhops, int sample_format,
                             void *hip_stream);
/* The same with every hop summed in the reference's own order (GLFER_SUBMEAN_EXACT above): what the
 * per-hop shim's prepare_audio() uses. */
int glfer_hip_submean_exact_device(const void *d_in, float *d_out, int hop, size_t nhops, int sample_format,
                                   void *hip_stream);

/* compute_floor (fft.c:240-294) for a batch of PSD rows on the device.
 * d_stats: [nframes][4] floats = {sig (max bin), floor, peak value, peak bin as float}. */
int glfer_hip_floor_device(const float *d_psd, size_t nframes, int bins, float *d_stats,
                           void *hip_stream);
/* the same over rows `pitch` floats apart (cfg.psd_pitch; pitch >= bins) */
int glfer_hip_floor_device_pitched(const float *d_psd, size_t nframes, int bins, int pitch, float *d_stats,
                                   void *hip_stream);

/* update_avg_* (avg.c:108-298) over consecutive PSD rows: the sliding sum over the last
 * `depth` frames per bin in [minbin,maxbin) and the three output normalisations.
 * The state starts empty (alloc_avg, avg.c:38-60) at row 0 of the call.
 *   d_avg  : [nframes][n_out] doubles (avgdata->avg after each frame; 1e-15 out of band)
 *   d_ret  : [nframes][4] doubles = {return value, peak bin, variance (sumavg), effdepth}
 */
int glfer_hip_avg_device(int avg_mode, const float *d_psd, size_t nframes, int bins, int n_out,
                         int depth, int minbin, int maxbin, int max0, double *d_avg,
                         double *d_ret, void *hip_stream);
/* Estimator AND moving average in one call: frames [first_frame, first_frame + nframes) of the stream as
 * glfer_hip_spectrogram_device computes them, followed by update_avg_* over those rows with the averaging state empty at
 * first_frame -- what source.c:141-158 and g_main.c:1153-1183 do per hop.  d_avg [nframes][n_out] and d_ret [nframes][4] as
 * glfer_hip_avg_device writes them (d_ret may be NULL); d_psd [nframes][N/2+1] receives the PSD rows themselves, or NULL: they
 * are then never stored.  n_out >= N/2+1 (the reference's avgdata is N wide, source.c:312).
 * The plain average (GLFER_AVG_PLAIN) over a window of up to four frames (the reference's default depth, glfer.c:295-296) of
 * a periodogram plan (FFT mode, N = 512..4096, no RA9MB / limiter, history from the stream; mean removal off, or the reference's own --
 * cfg.sub_mean = 1 with a hop of 2, 4, 8 or 16 sixteenths of the block: the hop means are taken first and given to the kernel) is taken INSIDE the
 * estimator launch, on the |X|^2 values while they are in registers: per frame 4 H bytes in and 8 n_out bytes out, no PSD row
 * in memory.  Every other case runs the two launches.  d_avg is identical, double for double, to glfer_hip_avg_device over
 * the rows (a window's sum of float bins is exact in a double unless a bin spans more than ~2^26 within the window); the band
 * mean in d_ret [.][0] is the same sum taken over the lanes in another order (equal to ~1e-15 relative), the peak bin equal.
 * GLFER_AVG_FUSED=0 in the environment forces the two launches (A/B runs). */
int glfer_hip_spectrogram_avg_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples, size_t first_frame,
                                     size_t nframes, int avg_mode, int depth, int minbin, int maxbin, int max0, int n_out,
                                     float *d_psd, double *d_avg, double *d_ret, void *hip_stream);

/* update_avg_* over the rows of nstreams independent streams, the state empty at row 0 of EACH stream.
 *   d_psd [nstreams][nframes][bins] floats, d_avg [nstreams][nframes][n_out] doubles, d_ret [nstreams][nframes][4] doubles.
 * Stream b's outputs equal glfer_hip_avg_device over d_psd + b*nframes*bins, double for double: the kernels' stream
 * dimension chooses chunks, window lead-ins and the fused or two-pass form from one stream's frame count, as that call
 * does.  The argument rules are glfer_hip_avg_device's; nstreams == 0 or nframes == 0: GLFER_OK, nothing launched.
 * One launch (two on the two-pass form) per 65 535 streams.  Asynchronous on hip_stream. */
int glfer_hip_avg_batch_device(int avg_mode, const float *d_psd, size_t nstreams, size_t nframes, int bins, int n_out,
                               int depth, int minbin, int maxbin, int max0, double *d_avg, double *d_ret, void *hip_stream);

/* glfer_hip_spectrogram_avg_device for nstreams streams laid out as glfer_hip_spectrogram_batch_device takes them
 * (d_streams, stream_pitch, nsamples, first_frame, nframes: same meaning and the same argument rules).
 *   d_psd [nstreams][nframes][bins] or NULL, d_avg [nstreams][nframes][n_out], d_ret [nstreams][nframes][4] or NULL.
 * Every output of stream b is bit for bit what glfer_hip_spectrogram_avg_device gives for that stream alone: the call
 * routes one stream's frames as that entry does (the average inside the estimator launch, its head frames and 2^24-frame
 * pieces, or the two launches) and makes every resulting launch cover the whole batch, so the launch count does not grow
 * with nstreams.  Where the rows themselves are not batched (N outside 256 .. 16384) they are computed stream by
 * stream, then averaged in one batched launch.  The argument rules of both entries apply (HP-ARMA refused, dense rows,
 * the band, n_out >= bins, an even pitch for s16 / u8); nstreams == 0 or nframes == 0: GLFER_OK, nothing launched.
 * Scratch: rows (without d_psd) and return values (without d_ret) of all streams at once on the two-launch route, cut into
 * groups of streams of at most 8 GiB of rows each.  Asynchronous on hip_stream. */
int glfer_hip_spectrogram_avg_batch_device(glfer_hip_plan *plan, const void *d_streams, size_t nstreams, size_t stream_pitch,
                                           size_t nsamples, size_t first_frame, size_t nframes, int avg_mode, int depth,
                                           int minbin, int maxbin, int max0, int n_out, float *d_psd, double *d_avg,
                                           double *d_ret, void *hip_stream);

/* The sliding sums alone: d_cum [nframes][n_out] = avgdata->cum after each frame (avg.c:114-127);
 * columns outside [minbin, maxbin) are left untouched. */
int glfer_hip_avg_cum_device(const float *d_psd, size_t nframes, int bins, int n_out, int depth,
                             int minbin, int maxbin, double *d_cum, void *hip_stream);

/* ---- Drift search: rows summed along straight lines of frequency drift ----
 * Every average above integrates along time at a fixed bin; a carrier that moves a few bins during a long integration (slow-CW
 * work: oscillator and path drift) is smeared over them.  These entries sum a block of T = `frames` consecutive rows along
 * every straight line from drift dmin to drift dmax (whole bins across the block's T - 1 steps) and keep, per bin, the largest
 * sum and the drift that gave it.
 *   P[f][k]   : float rows, k = 0 .. bins - 1 (bins <= 2^31 - 1025), `pitch` >= bins floats apart (rows of any entry above, as they lie on the device)
 *   frames    : T, 2 .. 4096
 *   step      : >= 1, rows from one block to the next (step = T: disjoint blocks; step < T: a moving search)
 *   dmin,dmax : dmin <= 0 <= dmax, -(T - 1) <= dmin, dmax <= T - 1, D = dmax - dmin + 1 <= 255
 * The offset of drift d at frame t, in integers, d t / (T - 1) rounded half away from zero:
 *     o(d, t) = sgn(d) ((2 |d| t + (T - 1)) div (2 (T - 1)))
 * so o(d, 0) = 0, o(d, T - 1) = d, o(-d, t) = -o(d, t), |o(d, t + 1) - o(d, t)| <= 1.  A run of F rows has
 * (F - T) / step + 1 blocks (none if F < T); block b starts at row b step.  Outputs, dense, any non-empty subset (NULL: not
 * written):
 *   d_sums  [nblocks][D][bins] floats : sums[b][d - dmin][k] = sum over t = 0 .. T - 1 of P[b step + t][k + o(d, t)], added in
 *             float in increasing t from +0.0f with plain adds; a term whose bin lies outside [0, bins) contributes nothing
 *             (the padding between bins and pitch and the next row are never read as data).  A block's values depend on its
 *             own T rows alone.
 *   d_best  [nblocks][bins] floats    : the largest of the D sums at k
 *   d_drift [nblocks][bins] shorts    : the d that gave it.  Among equal sums the smallest |d| wins and +d comes before -d: the
 *             rule is a scan in the order 0, +1, -1, +2, -2, ... that replaces on strict >, so a NaN on the zero-drift line
 *             gives NaN with drift 0, a NaN elsewhere never wins, and silence gives best = 0, drift = 0.
 * The waterfall and compute_floor entries take d_best rows as they are.
 * glfer_hip_drift_blocks and glfer_hip_drift_offsets touch no device: the block count (0 for frames outside 2 .. 4096 or
 * step == 0), and the check of frames / dmin / dmax (GLFER_OK or GLFER_E_ARG) with, where `offsets` is not NULL, o(d, t) at
 * offsets[(d - dmin) * frames + t].
 * glfer_hip_drift_device: blocks 0 .. nblocks - 1 of the nrows rows at d_rows.  One kernel (drift.hip): a workgroup streams a
 * block's rows through LDS, a tile of 256 bins and a halo of max(-dmin, dmax) each side, and a lane keeps up to 64 drifts'
 * sums in registers; more drifts are further passes over the block's rows inside the launch.  65 535 blocks a launch.
 * glfer_hip_drift_batch_device: the same over nstreams streams that share every size; stream b's rows at
 * d_rows + b * row_stride floats, its outputs at d_sums + b * sums_stride, d_best + b * best_stride, d_drift + b * drift_stride
 * elements (strides at least a stream's rows / outputs; ignored for one stream).  Stream b's outputs are bit for bit the single
 * entry's; one launch per 65 535 streams (per 65 535 blocks), the kernel's blockIdx.z the stream.
 * Neither entry allocates, uploads a table or waits for the device (the offsets are integer arithmetic in the kernel): both are
 * legal on a hip_stream that is being captured into a graph.
 * glfer_hip_spectrogram_drift_device: the rows are the plan's, for frames first_frame .. first_frame + (nblocks - 1) step + T - 1
 * of the stream, computed by glfer_hip_spectrogram_device into stream-ordered scratch (cfg.psd_pitch floats apart) and never
 * stored for the caller.  Every plan that entry takes.  The blocks go in pieces of whole blocks whose rows take at most half of
 * glfer_hip_scratch_limit's cap (one block at least); a piece's rows are computed from the multiple of GLFER_FRAME_ALIGN at or
 * below its first frame to the one at or above its last (inside the call's frames), so by rule (1) of "Cutting a stream" the
 * outputs are bit for bit those of the rows entry over the call's frames followed by glfer_hip_drift_device, whatever the cut.
 * It refuses a hip_stream that is being captured (scratch is taken per piece).
 * Arguments, in this order: GLFER_E_ARG for frames, step, dmin, dmax, bins or pitch out of range (and a NULL plan); GLFER_OK with
 * nothing launched for nblocks == 0 or no stream; GLFER_E_ARG for NULL rows, all three outputs NULL, nblocks above
 * glfer_hip_drift_blocks of the rows (frames past the stream), strides shorter than a stream, sizes that overflow size_t.
 * Not built: ragged, host, WAV and workers forms; a mean normalised by the count of in-range terms; fractional or curved
 * drifts (and no Taylor tree under this name: its paths are not these lines); drift sums of update_avg's double rows; more
 * than 255 drifts a call.  Asynchronous on hip_stream. */
size_t glfer_hip_drift_blocks(size_t nrows, size_t frames, size_t step);
int glfer_hip_drift_offsets(size_t frames, int dmin, int dmax, int *offsets /* [D][frames] */);
int glfer_hip_drift_device(const float *d_rows, size_t nrows, int bins, size_t pitch, size_t frames, size_t step, size_t nblocks,
                           int dmin, int dmax, float *d_sums, float *d_best, short *d_drift, void *hip_stream);
int glfer_hip_drift_batch_device(const float *d_rows, size_t nstreams, size_t row_stride, size_t nrows, int bins, size_t pitch,
                                 size_t frames, size_t step, size_t nblocks, int dmin, int dmax, float *d_sums, size_t sums_stride,
                                 float *d_best, size_t best_stride, short *d_drift, size_t drift_stride, void *hip_stream);
int glfer_hip_spectrogram_drift_device(glfer_hip_plan *plan, const void *d_stream, size_t nsamples, size_t first_frame, size_t frames,
                                       size_t step, size_t nblocks, int dmin, int dmax, float *d_sums, float *d_best, short *d_drift,
                                       void *hip_stream);

/* ---- display mapping: main_window_draw's column loop (g_main.c:1099-1236) over a batch ---- */
enum { GLFER_SCALE_LIN = 0, GLFER_SCALE_LIN_MAX0, GLFER_SCALE_LOG, GLFER_SCALE_LOG_MAX0 };   /* glfer.h:43 */
enum { GLFER_PAL_HSV = 0, GLFER_PAL_THRESH, GLFER_PAL_COOL, GLFER_PAL_HOT, GLFER_PAL_BW,
       GLFER_PAL_BONE, GLFER_PAL_COPPER, GLFER_PAL_OTD };                                      /* glfer.h:47 */

typedef struct {
  int scale_type;          /* opt.scale_type                                                   */
  int autoscale;           /* opt.autoscale                                                    */
  float overlap;           /* opt.data_blocks_overlap (first-buffer correction, g_main.c:1114) */
  float max_level_db;      /* opt.max_level_db / opt.min_level_db: used when autoscale is off  */
  float min_level_db;
  float thr_level;         /* opt.thr_level, percent                                           */
  int palette;             /* opt.palette                                                      */
  /* the state main_window_draw keeps between columns; updated by every call */
  int first_buffer;        /* glfer.first_buffer                                               */
  float display_max_lvl;   /* the two function statics of g_main.c:1081                        */
  float display_min_lvl;
  int psd_pitch;           /* floats from one row of d_psd to the next in glfer_hip_display_device / glfer_hip_waterfall_device /
                              glfer_hip_waterfall_map_device (0 = dense: `bins`); cfg.psd_pitch of the plan that wrote the rows */
} glfer_hip_display;

/* set_palette (g_main.c:651-762): 256 RGB triplets into host memory. */
int glfer_hip_palette(int palette, unsigned char colortab[768]);

/* One call = `nframes` consecutive calls of the mapping part of main_window_draw.
 *   d_psd    : [nframes][bins] float PSD rows (opt.averaging == NO_AVG), or NULL
 *   d_avg    : [nframes][bins] double rows of avgdata.avg (any averaging mode), or NULL
 *              -- exactly one of the two is given
 *   d_stats  : [nframes][4] as written by glfer_hip_floor_device (sig, floor are used)
 *   d_rgb    : [nframes][bins][3] bytes, pixel i of a column = bin bins-1-i (rgbbuf, n_zoom 1)
 *   d_lev    : [nframes][bins] shorts = levbuf column, or NULL
 *   d_levels : [nframes][4] floats = {display_max, display_min, display_max_lvl,
 *              display_min_lvl} used for each column, or NULL
 * disp->first_buffer / display_*_lvl are read as the incoming state and updated to the state
 * after the last column (the call synchronises the stream to read them back). */
int glfer_hip_display_device(glfer_hip_display *disp, const float *d_psd, const double *d_avg,
                             const float *d_stats, size_t nframes, int bins, unsigned char *d_rgb,
                             short *d_lev, float *d_levels, void *hip_stream);

/* compute_floor + update_avg_* + the mapping for a batch of PSD rows in one call (statistics,
 * level tracking, [moving average +] pixel map).  A single pass over a row is not possible: the level
 * tracking is a chain over the columns fed by every column's statistics, so a row is read once for
 * those and once to be mapped.  With averaging the averages are taken INSIDE the mapping kernel (the
 * levels come from compute_floor of the PSD rows, g_main.c:1109-1139, not from the average): no
 * averaged rows in memory at all.  Where that kernel does not apply (bands wider than 33 x 256 bins,
 * windows much deeper than its frame chunks; or GLFER_WATERFALL_FUSED=0) the averaged rows are scratch,
 * at most 4 GiB at a time, and the batch is walked in tiles of that many rows
 * (GLFER_WATERFALL_TILE=<rows> overrides).  avg_mode 0 = NO_AVG (the PSD rows are mapped), else
 * GLFER_AVG_* with depth/minbin/maxbin/max0 as glfer_hip_avg_device (the state starts empty at row
 * 0).  d_stats: [nframes][4] or NULL.  disp carries the level-tracking state in and out; the call
 * synchronises the stream per tile. */
int glfer_hip_waterfall_device(glfer_hip_display *disp, int avg_mode, int depth, int minbin, int maxbin,
                               int max0, const float *d_psd, size_t nframes, int bins,
                               unsigned char *d_rgb, short *d_lev, float *d_stats, void *hip_stream);

/* The waterfall of many independent streams in one call (a receiver per band or antenna, one display plan):
 *   d_psd   : [nstreams][nframes][pitch] floats, pitch = disps[0].psd_pitch (0: bins) -- what
 *             glfer_hip_spectrogram_batch_device writes
 *   d_rgb   : [nstreams][nframes][bins][3];  d_lev: [nstreams][nframes][bins] or NULL;  d_stats: [nstreams][nframes][4] or NULL
 *   disps   : [nstreams], stream b's carried state (first_buffer, display_max_lvl, display_min_lvl) in and out.  The options
 *             (scale_type, autoscale, overlap, max_level_db, min_level_db, thr_level, palette, psd_pitch) must be the same in
 *             every entry: GLFER_E_ARG otherwise, nothing launched, no state changed.
 * Stream b's rgb, lev, stats and state are byte for byte what glfer_hip_waterfall_device gives over d_psd + b*nframes*pitch
 * with a copy of disps[b] -- every avg_mode and max0, fused or staged average (GLFER_WATERFALL_FUSED and
 * GLFER_WATERFALL_TILE apply as there): the route, the frame tiles and the average-in-the-map shape are chosen from ONE
 * stream's frame count, and every launch covers the batch (the level walk, one wavefront chain per stream, blockIdx.y).  The
 * launch count does not grow with nstreams, save chunks of 65 535 streams and, staged, groups of streams whose averaged rows
 * stay within 4 GiB per tile.  One upload, one download of the states and one synchronisation per call.
 * Argument rules are glfer_hip_waterfall_device's; disps NULL with nstreams > 0: GLFER_E_ARG; nstreams == 0 or
 * nframes == 0: GLFER_OK, nothing launched.  On any error no entry of disps is modified.
 * Not covered: per-stream options (palettes, scales), batched host / WAV / workers waterfalls, several GPUs.  Streams of
 * unequal length: glfer_hip_waterfall_ragged_device below. */
int glfer_hip_waterfall_batch_device(glfer_hip_display *disps, size_t nstreams, int avg_mode, int depth, int minbin, int maxbin,
                                     int max0, const float *d_psd, size_t nframes, int bins, unsigned char *d_rgb, short *d_lev,
                                     float *d_stats, void *hip_stream);

/* The moving average and the waterfall of RAGGED rows: streams of unequal length, packed the way
 * glfer_hip_spectrogram_ragged_device writes them.  Stream b is rows [row_starts[b], row_starts[b + 1]).
 *   row_starts : HOST, [nstreams + 1], non-decreasing, consumed before the call returns -- what glfer_hip_ragged_frames and
 *                glfer_hip_spectrogram_ragged_device return
 * The single-stream kernels choose their shape from the stream's own frame count -- the chunk a block walks (128 frames,
 * halved down to 8 while there are fewer than 1024 chunks), and from it the fused or the two-pass form -- and a chunk restarts
 * its sliding sums from a direct sum, which equals the recurrence only while the sums are exact: a stream's last bits depend
 * on its OWN chunk length.  So the ragged kernels read a per-stream table (first row, frame count, the stream's own chunk
 * length, its first block), built on the host per call and uploaded to stream-ordered scratch; the blocks of a launch are one
 * flat list and a block finds its stream by bisection.  Streams that take the fused form and streams that take the two-pass
 * (waterfall: staged) form are two classes, each with its own launch set and table: the launch count of a call does not
 * depend on nstreams or on the lengths (save, staged, groups of streams whose averaged rows stay within 4 GiB).
 * compute_floor, the plain pixel map and the fixed levels work per row: they run over the packed rows as one run.
 * All three entries: nstreams == 0 or no rows at all: GLFER_OK, nothing written.  A decreasing row_starts, a NULL table, sizes
 * that overflow: GLFER_E_ARG before the device is touched.  A hip_stream that is being captured into a graph is refused
 * (GLFER_E_ARG): the tables come from host memory that is gone after the call.
 *
 * glfer_hip_avg_ragged_device: update_avg_* with the state empty at row 0 of each stream.  d_psd [rows][bins] (dense), d_avg
 * [rows][n_out] doubles, d_ret [rows][4] doubles or NULL.  Stream b's outputs equal glfer_hip_avg_device over its rows alone,
 * double for double.  Other arguments as glfer_hip_avg_device.
 *
 * glfer_hip_spectrogram_avg_ragged_device: the ragged rows (to d_psd, or to scratch when it is NULL), then the ragged average
 * over them.  The contract is the TWO-LAUNCH route: stream b's outputs are bit for bit glfer_hip_spectrogram_device followed
 * by glfer_hip_avg_device on that stream.  The average taken inside the estimator launch (glfer_hip_spectrogram_avg_device's
 * route for the plain average over up to four frames) is not built for ragged calls, and where that route sums in another
 * order (inexact sums only) the two entries differ in the last bits there.  The argument rules of both parents apply: HP-ARMA
 * plans and plans with a row pitch are refused, n_out >= bins, even offsets for s16 / u8.  row_starts: optional, out.
 *
 * glfer_hip_waterfall_ragged_device: glfer_hip_waterfall_batch_device for packed rows.  d_psd [rows][pitch] (pitch =
 * disps[0].psd_pitch, 0: bins), d_rgb [rows][bins][3], d_lev [rows][bins] or NULL, d_stats [rows][4] or NULL, all packed by
 * row_starts.  disps[b] carries stream b's state in and out; the options must be the same in every entry.  Stream b's pixels,
 * levbuf, statistics and returned state are byte for byte those of glfer_hip_waterfall_device over its rows with a copy of
 * disps[b]; a stream without rows leaves its disps[b] untouched.  Each stream takes the route the single entry would take for
 * its own length (the average inside the map, or staged: the ragged average into scratch, then the map);
 * GLFER_WATERFALL_FUSED=0 forces the staged class for every stream.  Where any stream's own route would cut it into tiles (a
 * stream longer than a tile; GLFER_WATERFALL_TILE below the longest stream) the call goes stream by stream through
 * glfer_hip_waterfall_device -- still byte-equal, one launch set per stream.  Argument errors and option mismatches:
 * GLFER_E_ARG, nothing launched, no entry of disps modified.  One download of the states and one synchronisation per call. */
int glfer_hip_avg_ragged_device(int avg_mode, const float *d_psd, size_t nstreams, const size_t *row_starts, int bins, int n_out,
                                int depth, int minbin, int maxbin, int max0, double *d_avg, double *d_ret, void *hip_stream);
int glfer_hip_spectrogram_avg_ragged_device(glfer_hip_plan *plan, const void *d_samples, size_t nstreams, const size_t *offsets,
                                            const size_t *lengths, int avg_mode, int depth, int minbin, int maxbin, int max0,
                                            int n_out, float *d_psd, double *d_avg, double *d_ret, size_t *row_starts,
                                            void *hip_stream);
int glfer_hip_waterfall_ragged_device(glfer_hip_display *disps, size_t nstreams, int avg_mode, int depth, int minbin, int maxbin,
                                      int max0, const float *d_psd, const size_t *row_starts, int bins, unsigned char *d_rgb,
                                      short *d_lev, float *d_stats, void *hip_stream);

/* The two halves of glfer_hip_waterfall_device for a waterfall whose columns live on several GPUs
 * (or are computed piece by piece).  The level tracking of main_window_draw (g_main.c:1111-1124) is
 * ONE chain over all columns, fed by the 16 bytes of compute_floor statistics per column; everything
 * else is per column.  So each GPU computes its rows and their statistics
 * (glfer_hip_spectrogram_device + glfer_hip_floor_device), the statistics meet on the host,
 *   glfer_hip_levels_host(disp, h_stats [n][4], n, h_levels [n][4], device)
 * walks them once (on `device`; disp's carried state in and out, exactly as
 * glfer_hip_display_device would leave it), and each GPU maps its own rows with its slice of the levels:
 *   glfer_hip_waterfall_map_device(disp, avg_mode, depth, minbin, maxbin, max0, d_batch, first, n,
 *                                  bins, d_levels [n][4], d_rgb, d_lev, stream)
 * maps rows [first, first + n) of the device batch d_batch ([.][bins] floats).  With averaging the
 * moving sums of the first rows reach back into the batch's rows BEFORE `first` -- a piece that is
 * not the start of the waterfall carries `depth` recomputed rows in front (recompute,
 * do not exchange); the state is empty at row 0 of the batch (alloc_avg, avg.c:38-60).  disp is
 * not modified. */
int glfer_hip_levels_host(glfer_hip_display *disp, const float *h_stats, size_t nframes, float *h_levels, int device);
int glfer_hip_waterfall_map_device(const glfer_hip_display *disp, int avg_mode, int depth, int minbin, int maxbin,
                                   int max0, const float *d_batch, size_t first, size_t nframes, int bins,
                                   const float *d_levels, unsigned char *d_rgb, short *d_lev, void *hip_stream);

/* Host samples -> waterfall columns: estimator, compute_floor and the display mapping on the
 * device, chunked through the same ring as glfer_hip_spectrogram_host; what comes back is
 * h_rgb [frames][bins][3] (and h_lev [frames][bins] shorts, or NULL): 3-5 bytes per bin over PCIe
 * instead of 4, and pixels instead of PSD rows.  disp carries the level-tracking state. */
int glfer_hip_waterfall_host(glfer_hip_plan *plan, glfer_hip_display *disp, const void *h_stream,
                             size_t nsamples, unsigned char *h_rgb, short *h_lev, size_t *nframes_out);

/* The waterfall over several GPUs (samples from a host array, or a WAV file): h_rgb [frames][bins][3]
 * (+ h_lev) identical to the one-GPU call's.  Three phases: every worker computes its frames' rows,
 * which stay on its GPU, and their compute_floor statistics; the statistics (16 bytes per column)
 * meet on the host and ONE walk gives every column its levels (glfer_hip_levels_host -- the level
 * tracking of g_main.c:1111-1124 is a chain over all columns); every worker maps its own rows with
 * its slice of the levels.  avg_mode != 0: update_avg_* (avg.c:108-298) inside the map; a worker whose
 * range starts at frame f > 0 RECOMPUTES the `depth` rows in front of it instead of receiving them
 *  -- the moving average crosses worker boundaries without an exchange.  disp carries
 * the level-tracking state in and out. */
int glfer_hip_waterfall_host_workers(const glfer_hip_config *cfg, const int *devices, int nworkers,
                                     glfer_hip_display *disp, int avg_mode, int depth, int minbin, int maxbin, int max0,
                                     const void *h_stream, size_t nsamples, unsigned char *h_rgb, short *h_lev,
                                     size_t *nframes_out);
int glfer_hip_waterfall_wav_workers(const glfer_hip_config *cfg, const int *devices, int nworkers,
                                    glfer_hip_display *disp, int avg_mode, int depth, int minbin, int maxbin, int max0,
                                    const char *path, size_t max_frames, unsigned char *h_rgb, short *h_lev,
                                    size_t *nframes_out, unsigned flags);
int glfer_hip_waterfall_wav_multi(const glfer_hip_config *cfg, unsigned device_mask, glfer_hip_display *disp,
                                  int avg_mode, int depth, int minbin, int maxbin, int max0, const char *path,
                                  size_t max_frames, unsigned char *h_rgb, short *h_lev, size_t *nframes_out,
                                  unsigned flags);

/* Device scratch the library keeps between calls.  Per-call scratch of 16 MiB and more (averaged
 * rows of a staged waterfall tile, the mean-corrected copy of a stream, big-block and LMP / F-test
 * spectra) comes from up to six blocks per device that the library allocates with hipMalloc and
 * KEEPS -- the stream-ordered pool costs milliseconds to seconds per GB-sized request on this stack
 * (profiles/r02_scratch_tail.txt).  That memory is invisible to the host application's own
 * allocator, so it is bounded and can be given back:
 *   glfer_hip_scratch_limit(bytes)        cap per device on kept bytes (default 16 GiB, or
 *                                         GLFER_SCRATCH_CAP_MB; 0 keeps nothing between calls).  Idle
 *                                         blocks are freed before a new one would exceed the cap, and
 *                                         all of them when a hipMalloc for a new block fails.
 *   glfer_hip_scratch_trim(device, keep)  frees idle kept blocks of `device`, smallest first, until at
 *                                         most `keep` bytes stay; waits for the work recorded on a
 *                                         block before freeing it; blocks in use by a running call
 *                                         stay.  Returns the bytes freed.  (The reference frees its
 *                                         buffers in fft_close, fft.c:297-306; a GUI host calls this
 *                                         when a waterfall is closed or the block size changes.)
 *   glfer_hip_scratch_held(device)        bytes kept right now.
 * GLFER_SCRATCH_CACHE=0 in the environment disables keeping altogether.
 * Besides the scratch blocks, ONE idle chunk ring of the host / file entries (two pinned sample buffers, two device buffers each
 * way; at most 2 GiB) is parked per device when its plan is destroyed and taken by the next plan that needs one -- the *_multi /
 * *_workers entries make a plan per worker and call, and allocating a ring costs 30-40 ms; glfer_hip_scratch_trim(device, 0)
 * frees it too.  The parked ring obeys the same switches as the blocks: nothing is parked with GLFER_SCRATCH_CACHE=0 or when the
 * ring is larger than the cap, glfer_hip_scratch_limit() below its size frees it, glfer_hip_scratch_held() counts it. */
size_t glfer_hip_scratch_trim(int device, size_t keep_bytes);
size_t glfer_hip_scratch_held(int device);
void glfer_hip_scratch_limit(size_t bytes);

const char *glfer_hip_strerror(int code);
/* text of the last HIP error seen by this thread ("" if none) */
const char *glfer_hip_last_hip_error(void);
/* library / kernel build description, e.g. "glfer_hip 0.1 gfx950" */
const char *glfer_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GLFER_HIP_H */
