/* lasr.h — C ABI of liblasr.so: the MI355X (gfx950) QuartzNet-CTC training hot path.
 *
 * The reference (kouyt5/lightning-asr) is pure Python and has NO FFI layer: its hot path runs
 * through torch / torchaudio operator calls.  Each entry point below therefore cites the
 * reference Python call site (path:line under the reference tree) whose arithmetic it replaces;
 * INTEGRATION.md shows the ctypes binding a maintainer adds at that call site.
 *
 * Conventions
 *   - plain C, POD arguments only: raw device pointers, int64 sizes, enums, hipStream_t as void*.
 *   - the CALLER owns every buffer (inputs, outputs, workspaces); the library allocates nothing
 *     on the device and never synchronises it.  All work is enqueued on `stream`.
 *   - return value: 0 = ok, <0 = LASR_E_* (bad argument/shape), >0 = hipError_t passthrough.
 *     lasr_last_error() returns a thread-local message for the last non-zero return.
 *   - activation layout is channels-last: a (B, C, T) reference tensor is stored [B][T][C]
 *     ("rows" n = b*T + t).  dtype of activations: LASR_F32 (parity mode) or LASR_BF16.
 *     Statistics, parameters, log-probs, CTC and the optimiser are always f32.
 */
#ifndef LASR_H
#define LASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LASR_VERSION 119   /* 101: lasr_mel_fwd_src / lasr_wav_read_batch / lasr_step_metrics / lasr_model_set_prefetch_src
                              102: LASR_LEN_LEAD (crop after pre-emphasis), lasr_wav_read_batch(lead_in), lasr_comm_timing*
                              103: lasr_ctc_beam_workspace_bytes / lasr_ctc_beam_decode (CTC prefix beam search)
                              104: lasr_arpa_* (ARPA n-gram LM), lasr_ctc_beam_decode_lm (beam search fused with it)
                              105: lasr_ctc_align_workspace_bytes / lasr_ctc_align (CTC forced alignment)
                              106: lasr_arpa_load_words / lasr_arpa_lexicon_info / lasr_ctc_beam_decode_wlm (word-level LM)
                              107: lasr_resample_* (sample-rate conversion, speed perturbation)
                              108: lasr_rir_bank_* / lasr_wave_augment* (noise and reverberation augmentation)
                              109: lasr_edit_align_workspace_bytes / lasr_edit_align_batch (substitution/deletion/insertion alignment)
                              110: lasr_dwconv_plan (which depthwise kernel form and grid a shape takes; launches nothing)
                              111: lasr_vad_* / lasr_segment_gather (voice-activity segmentation of long recordings)
                              112: lasr_hotword_* (phrase bank), lasr_ctc_beam_decode_bias / _lm_bias (hotword biasing)
                              113: lasr_ctc_kws_workspace_bytes / lasr_ctc_kws (CTC keyword search: phrases with time spans)
                              114: lasr_grad_accumulate / lasr_grad_accumulate_ranges (gradient accumulation over micro-batches)
                              115: lasr_bn_tail / lasr_bn_side / lasr_se_side: the BN entry points take one record; the _drop twins are gone
                              116: lasr_ema_state_bytes / lasr_ema_state_init / lasr_novograd_step_ema / lasr_ema_update (weight EMA)
                              117: lasr_clip_state_bytes / lasr_clip_state_init / lasr_novograd_step_clip (gradient clipping, non-finite guard)
                              118: lasr_ctc_beam_stream_* (resumable beam search: a sequence decoded chunk by chunk)
                              119: lasr_ctc_align_long* (banded forced alignment of long recordings) */

enum { LASR_F32 = 0, LASR_BF16 = 1 };
enum { LASR_ACT_NONE = 0, LASR_ACT_RELU = 1, LASR_ACT_SWISH = 2 };
enum { LASR_VARIANT_PLAIN = 0, LASR_VARIANT_CONTEXT = 1, LASR_VARIANT_CONTEXT_SE = 2,
       LASR_VARIANT_Q105 = 3 /* QuartNet105: ten residual blocks of five separable convolutions (models/QuartNet.py:175-224) */ };
enum {
  LASR_E_ARG = -1,      /* null pointer / negative size / unsupported enum */
  LASR_E_SHAPE = -2,    /* shape outside what the kernels are built for */
  LASR_E_WORKSPACE = -3, /* workspace too small */
  LASR_E_FORMAT = -4,    /* malformed input file (lasr_arpa_load) */
  LASR_E_UNSUPPORTED = -5, /* a well-formed input the library does not read (a KenLM binary model) */
  LASR_E_IO = -6          /* an input file that cannot be opened or read */
};

int lasr_version(void);
const char* lasr_last_error(void);

/* ---------------------------------------------------------------- features ----------------
 * data_module.py:150-174 AudioParser.parse_audio (torchaudio MelSpectrogram(16000, n_fft=512,
 * pad=32, win_length=320, hop_length=160, n_mels=64) + AmplitudeToDB('power'), :68-71):
 * dither (optional, noise passed in) -> pre-emphasis 0.97 -> |STFT|^2 -> HTK mel(64) ->
 * 10 log10(max(.,1e-10)) -> [SpecAugment rows/cols := 0, :97-122] -> (x-mean)/std (unbiased
 * over the utterance's own 64*T_b values, :171-172) -> zero padding past T_b (collate :222-248).
 */
int64_t lasr_mel_num_frames(int64_t n_samples); /* 1 + (n_samples + 64) / 160 */
size_t lasr_mel_workspace_bytes(int64_t B, int64_t T);
/* wave (B, L) f32, sample_lens (B) int32 valid samples per row (NULL = all L),
 * dither (B, L) f32 N(0,1) noise or NULL, aug (B,4) int32 {rect_x,w_x,rect_y,w_y} or NULL.
 * out_bft: (B, 64, T) f32 reference layout, may be NULL.
 * out_btf: (B, T, 64) channels-last in `dtype`, may be NULL.
 * frames_out (B) int32 = frames per utterance; pct_out (B) f32 = frames/T (collate :243).
 * normalize: 0 = stop at dB (no mean/std), 1 = full chain.                                   */
int lasr_mel_fwd(const float* wave, const int32_t* sample_lens, const float* dither, const int32_t* aug,
                 int64_t B, int64_t L, int normalize, float* out_bft, void* out_btf, int dtype,
                 int32_t* frames_out, float* pct_out, void* workspace, size_t workspace_bytes, void* stream);

/* lasr_mel_fwd with the samples as they sit in the wav file and the dither drawn on the device:
 *   wave_dtype LASR_WAVE_PCM16: wave is (B, L) int16 PCM; the kernel scales by 1/32768 (exact in f32 - the values
 *     torchaudio.load's normalisation hands data_module.py:153), so the H2D copy moves half the bytes;
 *   dither != NULL: explicit (B, L) N(0,1) noise, as lasr_mel_fwd;
 *   dither == NULL and dither_step != NULL: `y += 1e-5 * randn_like(y)` (data_module.py:155) is generated inside the kernel -
 *     Philox4x32-10 keyed by dither_seed with counter (sample / 4, utterance, *dither_step), Box-Muller - and *dither_step
 *     (device scalar, uint64) is incremented by the call, so a step replayed from a hipGraph draws fresh noise;
 *   both NULL: no dither.
 * lasr_dither_noise writes the noise a call with the same (seed, *step) uses: out (B, L) f32 (verification; the counter is
 * left untouched).                                                                                                   */
/* Crop AFTER dither + pre-emphasis (data_module.py:155-159: `y += noise; y = cat(y[0], y[1:] - 0.97 y[:-1]); y = sub_secquence(y)`):
 * the first sample of a crop that starts at file sample loc > 0 is y[loc] - 0.97 y[loc-1], not y[loc].  A caller that crops the RAW
 * waveform hands the sample before the crop over as a lead-in: row b = [x[loc-1], x[loc], ..., x[loc+n-1]] and
 * sample_lens[b] = n | LASR_LEN_LEAD.  The lead-in sample is dithered like every other sample (explicit noise: the row's first noise
 * value; generated noise: the row's first counter) and produces no output sample of its own.  n + 1 <= L.                     */
#define LASR_LEN_LEAD (1 << 30)
enum { LASR_WAVE_F32 = 0, LASR_WAVE_PCM16 = 1 };
/* pitch (round 5): elements between consecutive rows of `wave` (and of `dither`); 0 = L.  With pitch > L the batch sits in rows wider
 * than the L that defines the frame count T = 1 + (L + 64) / 160 (every utterance still ends at its own sample_lens[b] <= L, lead-in
 * sample included in the row: n + 1 <= pitch): a loader may keep ONE row pitch per frame-count class (static shapes for a captured
 * hipGraph) while T stays the reference's "pad to the longest utterance" value (data_module.py:222-248).                        */
typedef struct {
  const void* wave; int32_t wave_dtype; const float* dither; uint64_t dither_seed; uint64_t* dither_step; int64_t pitch;
} lasr_wave_src;
int lasr_mel_fwd_src(const lasr_wave_src* src, const int32_t* sample_lens, const int32_t* aug, int64_t B, int64_t L,
                     int normalize, float* out_bft, void* out_btf, int dtype, int32_t* frames_out, float* pct_out,
                     void* workspace, size_t workspace_bytes, void* stream);
int lasr_dither_noise(uint64_t seed, const uint64_t* step, int64_t B, int64_t L, float* out, void* stream);

/* AudioParser.spec_augment as a stand-alone call (data_module.py:97-122; inside the training chain the same zeros are written by
 * lasr_mel_fwd's `aug`): out = in with rows [rect_x, rect_x + w_x) and frames [rect_y, rect_y + w_y) of every (F, T) plane zeroed;
 * in / out (B, F, T) f32 (out may alias in), aug (B, 4) int32 = (rect_x, w_x, rect_y, w_y) drawn by the caller.        */
int lasr_spec_augment(const float* in, float* out, const int32_t* aug, int64_t B, int64_t F, int64_t T, void* stream);

/* (B, C, T) f32 reference layout -> [B][T][C] channels-last `dtype`   (models/QuartNet.py:154 squeeze) */
int lasr_bct_to_btc(const float* in, void* out, int dtype, int64_t B, int64_t C, int64_t T, void* stream);
int lasr_btc_to_bct(const void* in, int dtype, float* out, int64_t B, int64_t C, int64_t T, void* stream);

/* lens[b] = int32(trunc(f32(T) * pct[b]))   (models/QuartNet.py:311, train.py:76) */
int lasr_mask_lengths(const float* pct, int64_t B, int64_t T, int32_t* lens, void* stream);

/* ---------------------------------------------------------------- conv block pieces -------
 * models/QuartNet.py:29-39 SeprationConv.forward and :71-78 QuartNetBlock.forward.            */

/* depthwise conv1d, groups=C, zero padding k/2, no bias (models/QuartNet.py:19-21,30).
 * x [B][Tin][C] -> y [B][Tout][C], Tout = (Tin + 2*(k/2) - k)/stride + 1.  w (C, k) f32.
 * flip=1 correlates with the time-reversed taps (the data-gradient of a stride-1 conv).
 * addend (same shape as y, may be NULL) is added to the result.                               */
int lasr_dwconv_fwd(const void* x, const float* w, const void* addend, void* y, int dtype, int64_t B,
                    int64_t Tin, int64_t C, int k, int stride, int flip, void* stream);
/* dw (C, k) f32 = sum_{b,t} dy[b,t,c] * x[b, t*stride + j - k/2, c].  workspace: f32 partials. */
size_t lasr_dwconv_wgrad_workspace_bytes(int64_t B, int64_t Tout, int64_t C, int k);
int lasr_dwconv_wgrad(const void* x, const void* dy, float* dw, int dtype, int64_t B, int64_t Tin,
                      int64_t C, int k, int stride, void* workspace, size_t workspace_bytes, void* stream);

/* General GEMM on row-major device matrices, f32 accumulate on MFMA:
 *   C[M][N] = sum_k opA(A)[m][k] * opB(B)[n][k]  (+ bias[n]) (+ addend[m][n])
 * transA=0: A is [M][K] (K contiguous); transA=1: A is [K][M].  transB=0: B is [N][K]; 1: [K][N].
 * dtype_ab / dtype_c: LASR_F32 or LASR_BF16 (A and B share a dtype).
 * row_lens/rows_per_seq: if row_lens != NULL, output row m = b*rows_per_seq + t is written as
 *   zero when t >= row_lens[b]  (MaskCNN, models/QuartNet.py:309-321, applied BEFORE BN).
 * stats (2*N f32, may be NULL): stats[n] = sum_m C[m][n], stats[N+n] = sum_m C[m][n]^2 over the
 *   stored (masked, dtype-rounded) values, summed in a fixed order through `workspace`
 *   (feeds training-mode BatchNorm1d, :35).  Replaces pointwise_conv / reside.0 / last_cnn2.0 /
 *   decoder (models/QuartNet.py:31,63,146,275) and their autograd backward GEMMs.
 * split_k > 1 sums partial products through `workspace` (split_k*M*N f32), deterministic;
 *   it excludes row masking and statistics.                                                     */
size_t lasr_gemm_workspace_bytes(int64_t M, int64_t N, int split_k, int want_stats);
int lasr_gemm(const void* A, const void* B, void* C, int dtype_ab, int dtype_c, int64_t M, int64_t N,
              int64_t K, int transA, int transB, const float* bias, const void* addend,
              const int32_t* row_lens, int64_t rows_per_seq, float* stats, int split_k, void* workspace,
              size_t workspace_bytes, void* stream);

/* One or two independent GEMMs of the same kind (dtypes, transposition, split_k) in ONE launch: a unit's
 * main + residual 1x1 convolution (models/QuartNet.py:31 and :63), their two data gradients or their two
 * weight gradients.  Same semantics per problem as lasr_gemm (no addend).                              */
typedef struct {
  const void* A; const void* B; void* C;
  int64_t M, N, K;
  const float* bias; const int32_t* row_lens; int64_t rows_per_seq; float* stats;
} lasr_gemm_problem;
size_t lasr_gemm_batch_workspace_bytes(const lasr_gemm_problem* probs, int n_probs, int split_k);
int lasr_gemm_batch(const lasr_gemm_problem* probs, int n_probs, int dtype_ab, int dtype_c, int transA, int transB,
                    int split_k, void* workspace, size_t workspace_bytes, void* stream);

/* lasr_gemm with explicit leading dimensions (elements; 0 = the packed default) and no masking / statistics:
 * operands or results that are sub-blocks or row-padded copies of a larger matrix.  bf16 operands take the
 * aligned 16-byte path when the pitch is a multiple of 8 and the base 16-byte aligned, whatever M, N, K. */
int lasr_gemm_ld(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int dtype_ab, int dtype_c,
                 int64_t M, int64_t N, int64_t K, int transA, int transB, const float* bias, int split_k, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Eval-mode BN folded into the 1x1 convs:  for a unit  out = act(BN(mask(W u)) + BN_res(Wr x))  with
 * eval coefficients (a, b), (a2, b2):   out = act([mask(u) | x] . [a W | a2 Wr]^T + (b + b2)).
 *   lasr_fold_bn_weights_many: w_out [co][ci (+ci)] bf16 and bias_out [co] f32 for up to 32 units in one launch
 *       (coef / coef2 = the [a | b] vectors of lasr_bn_eval_coef_many; w_res = coef2 = NULL without a residual branch);
 *   lasr_gemm_dual: C[M][N] bf16 = act([A1 (rows past row_lens zeroed) | A2] . W^T + bias), A1 [M][K1], A2 [M][K2] bf16,
 *       W [N][K1+K2] bf16; K1, K2 multiples of 64, everything 16-byte aligned.  One GEMM, no separate BN pass.
 *       K2 = 0 with A2 = NULL: a unit without a residual branch, C = act(mask(A1) . W^T + bias).                  */
typedef struct {
  const float* w; const float* w_res; const float* coef; const float* coef2; void* w_out; float* bias_out; int64_t co, ci;
} lasr_fold_desc;
int lasr_fold_bn_weights_many(const lasr_fold_desc* descs, int n_descs, void* stream);
int lasr_gemm_dual(const void* A1, int64_t K1, const void* A2, int64_t K2, const void* W, const float* bias, void* C,
                   int64_t M, int64_t N, const int32_t* row_lens, int64_t rows_per_seq, int act, void* stream);

/* Deferred reductions.  The split-K weight-gradient GEMMs and the depthwise weight gradient end in a small
 * "sum the partial slabs" kernel each; a backward stage can instead leave the slabs where they are and sum all of
 * them with ONE launch at its end:
 *   lasr_gemm_batch_split_partials: lasr_gemm_batch(split_k > 1, f32 result) without the final sums;
 *       partials[i] -> [splits[i]][M_i*N_i] f32 inside `workspace` (which the caller must keep until the reduce);
 *   lasr_dwconv_wgrad_partials: lasr_dwconv_wgrad without the final sum; `workspace` holds [*n_partials][C*k];
 *   lasr_reduce_many: out[i] = sum_p partials[p*n + i] for up to 64 segments, f64 accumulation, fixed order. */
typedef struct { const float* partials; float* out; int64_t n; int32_t n_partials; } lasr_reduce_desc;
int lasr_reduce_many(const lasr_reduce_desc* descs, int n_descs, void* stream);
int lasr_gemm_batch_split_partials(const lasr_gemm_problem* probs, int n_probs, int dtype_ab, int transA, int transB,
                                   int split_k, void* workspace, size_t workspace_bytes, const float** partials,
                                   int* splits, void* stream);
/* Up to 32 bf16 weight-gradient problems C_i[M_i][N_i] = A_i^T B_i (A_i is [K][M_i], B_i is [K][N_i]: transA = transB = 1)
 * in ONE split-K launch; slabs[i] receives [splits[i]][M_i*N_i] f32 (splits[i] <= split_k), to be summed by
 * lasr_reduce_many.  Batching a whole backward stage makes the K slices longer and the slabs smaller. */
int lasr_gemm_multi_split_partials(const lasr_gemm_problem* probs, int n_probs, int split_k, float* const* slabs,
                                   int* splits, void* stream);
int lasr_dwconv_wgrad_partials(const void* x, const void* dy, int dtype, int64_t B, int64_t Tin, int64_t C, int k,
                               int stride, void* workspace, size_t workspace_bytes, int* n_partials, void* stream);
/* Both consumers of a unit's d(depthwise output) in one launch (stride 1): the weight-gradient partials of
 * lasr_dwconv_wgrad_partials(x, dy) and dx = lasr_dwconv_fwd(dy, w, addend, flip = 1).  Falls back to those two calls
 * for shapes / dtypes the fused MFMA kernel does not take.   (models/QuartNet.py:15-19 backward) */
int lasr_dwconv_bwd_fused(const void* x, const void* dy, const float* w, const void* addend, void* dx, int dtype,
                          int64_t B, int64_t T, int64_t C, int k, void* workspace, size_t workspace_bytes,
                          int* n_partials, void* stream);
/* Verification hook: the kernel forms and grids lasr_dwconv_fwd / lasr_dwconv_wgrad / lasr_dwconv_bwd_fused choose for a shape in
 * this process (the LASR_DW* switches are read once per process), computed by the launchers' own dispatch code.  Launches nothing.
 * Operands are taken as 16-byte aligned, the workspace as lasr_dwconv_wgrad_workspace_bytes sizes it.  Fields that do not apply to
 * the chosen form are 0 (bwd_form: -1 for stride 2, which has no data-gradient form).  Same argument errors as the launchers. */
enum { LASR_DW_FWD_STRIDED = 0, LASR_DW_FWD_F32 = 1, LASR_DW_FWD_MFMA = 2, LASR_DW_FWD_VALU = 3, LASR_DW_FWD_FMA = 4 };
enum { LASR_DW_WGRAD_STRIDED = 0, LASR_DW_WGRAD_VALU = 1, LASR_DW_WGRAD_MFMA = 2 };
enum { LASR_DW_BWD_TWO_LAUNCHES = 0, LASR_DW_BWD_TWO_KIND = 1, LASR_DW_BWD_UNI32 = 2, LASR_DW_BWD_UNI64 = 3 };
typedef struct {
  int32_t fwd_form;          /* LASR_DW_FWD_*: forward and (flip = 1) data gradient */
  int32_t nks, nset, gz_d;   /* MFMA forward: 32-wide K steps, 256-frame sets per time tile (1 = half tiles), gridDim.z */
  int32_t fwd_r;             /* strided forward: outputs per thread, 4 (64-frame tiles) or 8 */
  int32_t wgrad_form;        /* LASR_DW_WGRAD_* */
  int32_t zsplit;            /* MFMA weight gradient: time splits per utterance */
  int32_t ts;                /* VALU stride-1 weight gradient: time splits per workgroup (1..3) */
  int32_t bwd_form;          /* LASR_DW_BWD_*: what lasr_dwconv_bwd_fused launches */
  int32_t bwd_gz, bwd_tiles; /* unified backward: workgroups per utterance and channel group, 256-frame tiles per utterance */
  int32_t bwd_wgs, bwd_wgs_launched;   /* unified backward: workgroups with work, and gridDim.x (padded to groups of 16) */
} lasr_dwconv_plan_info;
int lasr_dwconv_plan(int64_t B, int64_t T, int64_t C, int k, int stride, int dtype, lasr_dwconv_plan_info* plan);

/* lasr_gemm_batch that leaves each problem's BN partial sums UNREDUCED in the workspace (no split-K):
 * for every problem with stats != NULL, stat_partials[i] points at [stat_tiles[i]][2][N] f32 inside
 * `workspace` (valid until the workspace is reused) and problem.stats itself is not written.
 * lasr_bn_finalize_partials consumes them: 1 launch instead of 2 reductions + 2 finalizes per unit. */
int lasr_gemm_batch_partials(const lasr_gemm_problem* probs, int n_probs, int dtype_ab, int dtype_c, int transA,
                             int transB, void* workspace, size_t workspace_bytes, const float** stat_partials,
                             int* stat_tiles, void* stream);

/* Training-mode BatchNorm1d(eps) statistics -> affine coefficients (models/QuartNet.py:24,35):
 * mean = s/n, var = q/n - mean^2 (biased); coef[c] = gamma*rstd, coef[C+c] = beta - mean*gamma*rstd;
 * saved[c] = mean, saved[C+c] = rstd; running_mean/var updated with momentum (unbiased var) when
 * non-NULL.  training=0: coefficients from the running statistics, stats ignored.              */
int lasr_bn_finalize(const float* stats, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, float* coef, float* saved, int64_t C, int64_t n_rows, float eps,
                     float momentum, int training, void* stream);
/* Eval mode (training = 0) coefficients of up to 64 BN layers in one launch: coef[c] = gamma*rstd,
 * coef[C+c] = beta - running_mean*gamma*rstd with rstd = 1/sqrt(running_var + eps); the running statistics are read only. */
typedef struct {
  const float* gamma; const float* beta; const float* running_mean; const float* running_var; float* coef; int64_t C;
} lasr_bn_eval_desc;
int lasr_bn_eval_coef_many(const lasr_bn_eval_desc* descs, int n_descs, float eps, void* stream);

/* Training-mode lasr_bn_finalize for one or two BN layers of the same width (a unit's main and residual
 * branch) straight from GEMM partial sums: fixed-order f64 column reduction + the same arithmetic, one
 * launch.  stats (optional) receives the reduced [sum | sumsq] (2C f32).   (models/QuartNet.py:24,35) */
typedef struct {
  const float* partials; int n_partials;          /* [n_partials][2][C] */
  const float* gamma; const float* beta; float* running_mean; float* running_var;
  float* coef; float* saved; float* stats;
} lasr_bn_branch;
int lasr_bn_finalize_partials(const lasr_bn_branch* branches, int n_branches, int64_t C, int64_t n_rows, float eps,
                              float momentum, void* stream);
/* nn.Dropout(p) of SeprationConv / last_cnn2 (models/QuartNet.py:26,38,149) folded into the BN-apply kernels as a counter-based
 * (Philox4x32-10) mask: forward and both backward passes regenerate it from (seed, *step, unit, element index); no mask tensor
 * exists.  step: device scalar holding the index of the current training forward (lasr_mask_lengths_step bumps it as the first
 * launch of a forward, so replayed graphs draw fresh masks); unit: distinct per layer.  A residual unit drops its MAIN branch
 * before the add (the Dropout at the end of its SeprationConv), first_cnn / last_cnn2 drop after the activation.  Kept
 * elements are scaled by 1/(1-p).  step = NULL or p = 0: off.  lasr_dropout_mask writes the mask itself (1 = kept) for
 * verification against a CPU reference.                                                                                 */
typedef struct { const uint64_t* step; uint64_t seed; uint32_t unit; float p; } lasr_dropout;
int lasr_mask_lengths_step(const float* pct, int64_t B, int64_t T, int32_t* lens, uint64_t* step_counter, void* stream);
int lasr_dropout_mask(const lasr_dropout* dropout, int64_t n, uint8_t* keep, void* stream);

/* The tail every conv unit ends in,  out = act( BN(y) * se_scale[b][c] + BN_res(y2) )  with optional dropout and length masking
 * (BN-apply + SE scale + residual add + ReLU: models/QuartNet.py:35-37,74-77; ContextSE :55), described ONCE: the forward and every
 * backward entry point below take this record and read the fields they need (a field an entry point does not list is ignored).
 * "No residual branch" is res.y == NULL and nothing else: the other fields of `res` are then not looked at.                   */
typedef struct {                 /* one BatchNorm branch of the tail */
  const void* y;                 /* pre-BN tensor [B][T][C] in `dtype` */
  const float* coef;             /* [2][C] scale | shift, as lasr_bn_finalize leaves them */
  const float* saved;            /* [2][C] mean | rstd                                          (backward) */
  const float* gamma;            /* [C]                                                         (backward apply) */
  const float* beta;             /* [C]                                                         (lasr_bn_se_bwd, main only) */
  float* sums;                   /* reduced [2][C] sums between stats and apply; NULL: fused hand-over through the workspace */
  void* dy;                      /* [B][T][C] gradient of y                                     (backward apply) */
  float* dgamma; float* dbeta;   /* [C] parameter gradients                                     (backward apply) */
} lasr_bn_side;
typedef struct {
  int dtype; int act;            /* LASR_F32 / LASR_BF16 of y, y2, dout, dy, out; LASR_ACT_* */
  int64_t B, T, C;
  lasr_bn_side main, res;
  const void* dout;              /* [B][T][C] gradient of out                                   (backward) */
  const float* se_scale;         /* [B][C] f32, may be NULL: no SE scale */
  const float* se_grad;          /* [B][C] f32, may be NULL: extra per-(b,c) gradient added to d*se (SE pooled path) */
  const int32_t* row_lens;       /* (B), may be NULL: rows t >= row_lens[b] of main.dy are zeroed (`res` is never masked) */
  lasr_dropout dropout;          /* step == NULL or p == 0: off */
} lasr_bn_tail;
int lasr_bn_act_fwd(const lasr_bn_tail* tail, void* out, void* stream);   /* reads y, coef of both sides, se_scale, dropout */
/* lasr_bn_finalize_partials + lasr_bn_act_fwd (no SE scale, no dropout) in ONE launch, bf16 and C a multiple of 64: workgroups of
 * 64 channels x a chunk of rows fold the coefficients of their own channels from the partial sums in their prologue (the finalize
 * launch's arithmetic in the same order: the same bits) and apply them; coef / saved / stats / the running statistics of `branches`
 * are written as lasr_bn_finalize_partials writes them.  Of the record only y of both sides, dtype, act and the shape are read;
 * n_branches = 2 with res.y (main, residual), 1 without; n_rows = B*T.                                                        */
int lasr_bn_act_fwd_partials(const lasr_bn_branch* branches, int n_branches, float eps, float momentum, const lasr_bn_tail* tail,
                             void* out, void* stream);

/* Backward of the tail + BatchNorm backward, two passes over the activations:
 * pass 1 (stats): d = dout * act'(.) ; main.sums[0..C) = sum d*se, [C..2C) = sum d*se*yhat for branch 1
 *                 and the same for branch 2 in res.sums (se=1 there); yhat = (y-mean)*rstd.
 * pass 2 (apply): dy = gamma*rstd * (d*se - s1/n - yhat*s2/n), rows t >= row_lens[b] zeroed for
 *                 branch 1 only (the residual branch is never masked, models/QuartNet.py:75).
 * The pre-activation is rebuilt from y/y2 and the coefficients, so the forward output is not read.
 * dgamma = s2, dbeta = s1 are written by pass 2 (f32, may be NULL).
 * se_grad ([B][C] f32, may be NULL): extra per-(b,c) gradient added to d*se (SE pooled path).
 * Fused hand-over: call stats and apply with main.sums = res.sums = NULL and the SAME workspace
 * (lasr_bn_bwd_workspace_bytes): the per-block partial sums stay in the workspace and pass 2
 * reduces them while folding its per-channel constants (one launch less, no f32 round trip).
 * stats reads dout, y / coef / saved of both sides, se_scale, se_grad, dropout and writes sums; apply reads gamma, sums, row_lens
 * as well and writes dy, dgamma, dbeta of both sides.                                           */
size_t lasr_bn_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C);
int lasr_bn_act_bwd_stats(const lasr_bn_tail* tail, void* workspace, size_t workspace_bytes, void* stream);
int lasr_bn_act_bwd_apply(const lasr_bn_tail* tail, void* workspace, size_t workspace_bytes, void* stream);
size_t lasr_bn_bwd_apply_workspace_bytes(int64_t C);   /* folded per-channel constants, 10*C f32 */

/* The excite MLP of a ContextSE unit (models/QuartNetContextSE.py:8-23), as its backward takes it: hidden (B,C/8), pooled (B,C) from
 * lasr_se_fwd, ysum (B,C) = sum_t y from lasr_seqsum (lasr_bn_se_bwd only), W1 (C/8,C), W2 (C,C/8); outputs seg (B,C), dW1, dW2. */
typedef struct {
  const float* hidden; const float* pooled; const float* ysum; const float* W1; const float* W2;
  float* seg; float* dW1; float* dW2;
} lasr_se_side;
/* Backward of a ContextSE unit's  out = act(BN(y) * se + BN_res(y2))  (models/QuartNetContextSE.py:19-23,54-57) in TWO passes over
 * (dout, y, y2): per-utterance raw sums -> SE-scale gradient by algebra (gamma*sum(d*xhat) + beta*sum(d)) -> excite-MLP backward
 * (se->seg [B][C], dW1, dW2) -> BN-backward constants -> dy, dy2, dgamma, dbeta.  se->seg takes the place of tail->se_grad, and
 * the sums go through the workspace.  Replaces lasr_se_bwd + lasr_bn_act_bwd_stats + lasr_bn_act_bwd_apply (three passes) for the
 * SE units.                                                                                                                  */
size_t lasr_bn_se_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C);
int lasr_bn_se_bwd(const lasr_bn_tail* tail, const lasr_se_side* se, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- SE + BiLSTM context --------
 * models/QuartNetContextSE.py:8-23,55  SELayer(reduction=8, no bias): s = sigmoid(W2 relu(W1 mean_T(BN(y)))),
 * mean over ALL T' frames.  BN is affine per channel, so the squeeze needs only sums[b][c] = sum_t y[b,t,c]
 * (lasr_seqsum) and the BN coefficients; the scale is applied inside lasr_bn_act_fwd (se_scale).          */
int lasr_seqsum(const void* x, int dtype, int64_t B, int64_t T, int64_t C, float* sums, void* stream);
/* pooled (B,C) = coef_a*sums/T + coef_b ; hidden (B,C/8) = relu(W1 pooled) ; scale (B,C) = sigmoid(W2 hidden) */
int lasr_se_fwd(const float* sums, const float* coef, const float* W1, const float* W2, int64_t B, int64_t T, int64_t C,
                float* pooled, float* hidden, float* scale, void* stream);
/* Backward of the excite path: se->seg (B,C) = gradient reaching every frame of the BN output through the pooled
 * mean (feed it to lasr_bn_act_bwd_* as se_grad), dW1 (C/8,C), dW2 (C,C/8).  Of the tail (lasr_bn_tail, above) it reads dout, y and
 * coef of both sides, se_scale (required) and dropout.  C a multiple of 32; the whole batch is handled by two launches whose
 * per-workgroup tables (B x C/8 floats and change) must fit 64 KB of LDS (B <= ~200 at C = 512). */
size_t lasr_se_bwd_workspace_bytes(int64_t B, int64_t C);
int lasr_se_bwd(const lasr_bn_tail* tail, const lasr_se_side* se, void* workspace, size_t workspace_bytes, void* stream);

/* models/QuartNetContext.py:171-173,186-199: pack_padded_sequence -> nn.LSTM(256, 40, bidirectional) ->
 * pad_packed_sequence.  gx_f/gx_r (B,T,160) f32 = x W_ih^T per direction (lasr_gemm; biases are added here),
 * gate order i,f,g,o, reverse direction starts at each utterance's last valid frame, outputs zero for
 * t >= lens[b].  Writes h into columns [col0, col0+80) of a [B][T][ld_out] tensor (the cat() of :173).
 * saved: lasr_bilstm_saved_bytes(B,T) of f32 state for the backward pass.                                  */
size_t lasr_bilstm_saved_bytes(int64_t B, int64_t T);
int lasr_bilstm_fwd(const float* gx_f, const float* gx_r, const float* whh_f, const float* whh_r, const float* bih_f,
                    const float* bhh_f, const float* bih_r, const float* bhh_r, const int32_t* lens, int64_t B, int64_t T,
                    void* out, int dtype, int64_t ld_out, int64_t col0, float* saved, void* stream);
/* dout: columns [col0, col0+80) of a [B][T][ld_dout] gradient.  dg_f/dg_r (B,T,160) f32 = gradient w.r.t. the gate
 * pre-activations (=> dW_ih = dg^T x, db = colsum(dg), dx = dg W_ih by lasr_gemm), dwhh_f/dwhh_r (160,40).  */
size_t lasr_bilstm_bwd_workspace_bytes(int64_t B);
int lasr_bilstm_bwd(const void* dout, int dtype, int64_t ld_dout, int64_t col0, const float* whh_f, const float* whh_r,
                    const int32_t* lens, int64_t B, int64_t T, const float* saved, float* dg_f, float* dg_r, float* dwhh_f,
                    float* dwhh_r, void* workspace, size_t workspace_bytes, void* stream);
/* dst[n][dcol0+c] (+)= src[n][scol0+c], c < ncols, with dtype conversion (torch.cat / its backward slice, :173) */
int lasr_copy_cols(const void* src, int src_dtype, int64_t ld_src, int64_t scol0, void* dst, int dst_dtype, int64_t ld_dst,
                   int64_t dcol0, int64_t rows, int64_t ncols, int accumulate, void* stream);

/* ---------------------------------------------------------------- head + loss --------------
 * models/QuartNet.py:287-290 log_softmax over classes; train.py:76-78,196 CTCLoss(blank=C-1,
 * reduction='none', zero_infinity=False) and the batch mean; utils/asr_metrics.py:138-171.     */

/* logits [N][C] f32 -> logp [N][C] f32 (may alias logits), argmax (N) int32 (may be NULL).
 * Ties resolve to the lowest class id, as torch.argmax does on CPU.                            */
int lasr_log_softmax(const float* logits, float* logp, int32_t* argmax, int64_t N, int64_t C, void* stream);
/* grad_logits = grad_logp - exp(logp) * sum_c grad_logp   (autograd of F.log_softmax) */
int lasr_log_softmax_bwd(const float* logp, const float* grad_logp, float* grad_logits, int64_t N, int64_t C,
                         void* stream);

/* Longest label sequence the CTC heads take (lasr_ctc_loss, lasr_ctc_loss_mel, lasr_ctc_loss_lean, the model's loss): a
 * feasible sample needs S + repeats <= T', so 2047 covers every transcript of a 40 s clip (T' = 2001).  Above it the
 * workspace functions return 0 and the losses LASR_E_SHAPE. */
#define LASR_CTC_MAX_LABELS 2047
/* alpha + beta lattices + the same-label chains.  Rows hold 64 * 4/8/16 states for S_max <= 511 and 1024 * W states for
 * longer labels (W = ceil((2 S_max + 1) / 1024) = 2..4 waves per direction): for B = 32, T' = 2001 and S_max = 600 (W = 2)
 * that is about 1 GB.  0 when S_max > LASR_CTC_MAX_LABELS. */
size_t lasr_ctc_workspace_bytes(int64_t B, int64_t T, int64_t S_max);
/* logp (B, T, C) f32 log-probs; targets (B, S_max) int64 zero padded; in_lens/tgt_lens (B) int32.
 * nll (B) f32 per-sample negative log-likelihood (+inf when infeasible).
 * If grad != NULL: grad (B,T,C) f32 = gscale[b] * (exp(logp) - occupancy): exactly what torch's
 *   CTCLoss backward returns for grad_output = gscale.  Its class-sum is 0, so log_softmax backward
 *   maps it to itself: it is also d/d(logits).  Rows t >= in_lens[b] are zero; rows of an infeasible
 *   sample are NaN (zero_infinity=False).  gscale (B) f32 or NULL (= 1/B: batch mean, train.py:77).
 *   S_max <= LASR_CTC_MAX_LABELS (2047).  Up to 511 the 2S+1 states of a direction are held 4/8/16 per lane of one
 *   wave; longer labels run each direction on 2..4 waves of 16 states per lane.                     */
int lasr_ctc_loss(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens,
                  int64_t B, int64_t T, int64_t C, int64_t S_max, int blank, float* nll, float* grad,
                  const float* gscale, void* workspace, size_t workspace_bytes, void* stream);
/* lasr_ctc_loss for one batch and lasr_mel_fwd for ANOTHER batch's waveforms in one launch sequence: the lattice kernel
 * keeps 32 workgroups busy for ~0.1 ms of dependent steps, the feature transform (2 016 workgroups) fills the other CUs
 * meanwhile (one grid: lattice workgroups first).  Same results as the two calls; falls back to them for shapes the
 * fused grid does not take (more than 127 labels, C % 4 != 0, emissions over 78 KB).  This is the data-loader prefetch of
 * data_module.py's workers: the features of step i+1 are produced while step i computes its loss. */
int lasr_ctc_loss_mel(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens,
                      int64_t B, int64_t T, int64_t C, int64_t S_max, int blank, float* nll, float* grad,
                      const float* gscale, void* ctc_workspace, size_t ctc_workspace_bytes, const float* wave,
                      const int32_t* sample_lens, const float* dither, const int32_t* aug, int64_t Bm, int64_t L,
                      int normalize, float* out_bft, void* out_btf, int dtype, int32_t* frames_out, float* pct_out,
                      void* mel_workspace, size_t mel_workspace_bytes, void* stream);

/* CTC forced alignment: the Viterbi (max-product) path of the lasr_ctc_loss lattice, its backtrace and the per-label spans, in
 * one launch of one workgroup per utterance on `stream`; nothing is allocated or synchronised, so the call can be captured.
 * Arguments and states as lasr_ctc_loss: logp (B, T, C) f32, targets (B, S_max) int64 (clamped into the row on the device),
 * tgt_lens (B) int32 clamped to [0, S_max], in_lens (B) int32 clamped to [0, T] or NULL (= T); state 2i+1 is label i, even
 * states are blanks, the skip s-2 -> s exists only between different labels.
 *   v[0][s] = logp[0][cls(s)] for s in {0, 1}, dead otherwise; v[t][s] = max(stay, step, skip) + logp[t][cls(s)] in f32 (one
 *   rounding per state per frame).  Backpointer: the candidate that attains the max, on equality stay, then step, then skip.
 *   Final state: 2S if v[Tb-1][2S] >= v[Tb-1][2S-1] or S == 0, else 2S-1.  A final score that is not above -5e29 (a dead state,
 *   -inf or NaN) is infeasible - in particular Tb < S + (adjacent equal labels): score -inf, every index output -1, frame_logp 0.
 *   Tb == 0: score 0 when S == 0, infeasible otherwise.
 * score (B) f32; frame_state (B, T) int32: the state 0..2S of every frame, -1 past in_lens; frame_logp (B, T) f32: logp of that
 * state's class, 0 where frame_state is -1; label_start / label_end (B, S_max) int32: first frame of label i and one past its
 * last, -1 for i >= tgt_lens.  S_max may be 0 (targets and the label outputs may then be NULL).
 * The workspace holds the backpointers, 2 bits per state (T rows of 64 dwords per wave and utterance); S_max above
 * LASR_CTC_MAX_LABELS: workspace bytes 0 and LASR_E_SHAPE, nothing launched. */
size_t lasr_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t S_max);
int lasr_ctc_align(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens,
                   int64_t B, int64_t T, int64_t C, int64_t S_max, int blank, float* score, int32_t* frame_state,
                   float* frame_logp, int32_t* label_start, int32_t* label_end, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Forced alignment of LONG recordings: lasr_ctc_align on a band of `band` = W states that follows the path, for transcripts far
 * above LASR_CTC_MAX_LABELS (an hour of speech is T ~ 180 000 frames and ~50 000 labels; its full lattice is 1.8e10 cells).  One
 * launch of one workgroup per recording on `stream`; nothing is allocated or synchronised, so the call can be captured.
 * The lattice, the emission rule, the max, the tie rule (stay, then step, then skip), the end rule, the dead-state convention and
 * the outputs score / frame_state / frame_logp / label_start / label_end are those of lasr_ctc_align, word for word.  The band:
 *   W is a multiple of 256 in [256, 4096] or a multiple of 1024 up to LASR_CTC_ALIGN_LONG_MAX_BAND.  G = 64 states
 *   (lasr_ctc_align_long_granule), R = 32 frames (lasr_ctc_align_long_period).
 *   Frame t keeps states [lo_t, lo_t + W).  lo_0 = 0; lo changes only at frames t0 that are positive multiples of R.  There
 *     a      = the live state (value above -5e29, state below 2S+1) of row t0-1 with the largest value, the lowest state on ties;
 *              lo_prev when no state is live
 *     centre = floor((a - W/2) / G) * G
 *     reach  = ceil((s_min(te) - (W-1)) / G) * G with te = min(t0 + R - 1, Tb - 1) and s_min(t) = 2S-1 - 2 (Tb-1-t), the lowest
 *              state from which the end can still be reached
 *     lo     = min(max(lo_prev, centre, reach), ceil(max(0, 2S+1 - W) / G) * G)
 *   A candidate read from a state outside the previous frame's band is dead; states >= 2S+1 are dead.  W/2 - G >= 2R: a path that
 *   advances two states per frame for a whole period stays inside the band above the argmax.
 *   A band of at least 2S+1 states never moves and the result is lasr_ctc_align's, bit for bit.  A narrower band prunes: it can
 *   return a feasible path that is not the best one, without any flag, or lose every path (status 2).
 * status (B) int32: 0 aligned; 1 infeasible by count (Tb < S + adjacent equal labels, or Tb == 0 < S); 2 lost (feasible by count,
 * but neither end state is live in the last frame's band).  On 1 and 2 the other outputs are the infeasible ones of
 * lasr_ctc_align.  band_lo (B, T) int32: lo_t for t < Tb (by the rule above whatever the status), -1 from Tb on.
 * S_max <= LASR_CTC_ALIGN_LONG_MAX_LABELS; every offset into logp, the outputs and the workspace is 64-bit (no T * C < 2^31 bound).
 * The workspace holds the backpointers, 2 bits per banded state: W / 4 bytes per frame (an hour at W = 4096: about 180 MB).
 * Before any launch: a null pointer (or a workspace that is not 4-byte aligned) LASR_E_ARG; a band, blank, S_max or shape outside
 * the above LASR_E_SHAPE; a workspace below lasr_ctc_align_long_workspace_bytes (0 for arguments the call refuses)
 * LASR_E_WORKSPACE. */
#define LASR_CTC_ALIGN_LONG_MAX_LABELS (1 << 24)
#define LASR_CTC_ALIGN_LONG_MAX_BAND 8192
int64_t lasr_ctc_align_long_period(void);
int64_t lasr_ctc_align_long_granule(void);
size_t lasr_ctc_align_long_workspace_bytes(int64_t B, int64_t T, int64_t S_max, int64_t band);
int lasr_ctc_align_long(const float* logp, const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens,
                        int64_t B, int64_t T, int64_t C, int64_t S_max, int blank, int64_t band, float* score,
                        int32_t* frame_state, float* frame_logp, int32_t* label_start, int32_t* label_end, int32_t* status,
                        int32_t* band_lo, void* workspace, size_t workspace_bytes, void* stream);

/* CTC keyword search: where in each utterance is each of K phrases said, and how well?  The third member of the lattice family:
 * a max-product walk like lasr_ctc_align's, with a free start and a free end.  One wave per (utterance, keyword) pair, the
 * picking of the hits in the same launch, everything on `stream`; nothing is allocated or synchronised.
 * logp (B, T, C) f32 log-probabilities, finite or -inf; in_lens (B) int32 clamped to [0, T], or NULL (= T); the keyword bank in the
 * form lasr_hotword_build takes, but on the DEVICE: kw_labels int32 concatenated, kw_offsets (K + 1) int32 ascending offsets
 * into it.  L_max in [1, LASR_KWS_MAX_LABELS] is the caller's bound on the longest phrase.  The device clamps every phrase start
 * into [0, kw_offsets[K] - 1], every length into [1, min(L_max, labels left)] and every label into [0, C - 1], so that bad data
 * cannot become an out-of-bounds access (kw_labels must hold at least one entry).
 * For utterance b with Tb frames and a keyword with labels l_0 .. l_{L-1}:
 *   States j = 0 .. 2L-2: even j is label l_{j/2}, odd j a blank between two labels; no leading or trailing blank (those are
 *   the background's).  skip_ok(j) holds for even j >= 2 iff l_{j/2} != l_{j/2-1}.
 *   Filler-normalised emission: m_t = max_c logp[b,t,c] (the blank included), e_t(j) = logp[b,t,cls(j)] - m_t, one f32
 *   subtraction, so e_t(j) <= 0: a path's score is its log-likelihood ratio against the greedy path over the same frames.
 *   Each state carries (v, s): an f32 score and the frame at which its path entered state 0.  Candidates at frame t: stay
 *   (v,s)_{t-1}(j); step (v,s)_{t-1}(j-1) for j >= 1; skip (v,s)_{t-1}(j-2) if skip_ok(j); fresh (0, t) for j == 0 only.  The
 *   best candidate has the larger v, on equal v the smaller s (ties go to the earliest start; a fresh start loses ties to
 *   staying).  v_t(j) = best.v + e_t(j), one f32 add; s_t(j) = best.s.  Before t = 0 every state is dead.
 *   End trace: E_t = v_t(2L-2), S_t = s_t(2L-2) (L = 1: state 0 is both ends).
 * Hits of (b, k), t ascending, thr = (float)threshold * (float)L (one f32 multiply): frame t is a candidate iff E_t >= thr, its
 * span [S_t, t+1), its score E_t.  One hit is pending.  A candidate whose start is below the pending hit's end overlaps it and
 * replaces it iff its score >= the pending score (the later candidate wins ties); one that does not overlap emits the pending
 * hit and becomes pending; the last pending hit is emitted at the end.  Emitting writes slot n only while n < max_hits but
 * always counts: n_hits (B, K) may exceed max_hits (the convention of lasr_vad_segment's n_segs).  hit_span (B, K, max_hits, 2)
 * int32, hit_score (B, K, max_hits) f32; unwritten slots hold (-1, -1) and 0.
 * Best of each pair, whatever the threshold: best_score (B, K) = max_t E_t, on ties the latest t; best_span (B, K, 2) that
 * frame's [S_t, t+1).  Dead states hold a finite sentinel: an end score not above -5e29 (a dead state, -inf, NaN) is not live;
 * with no live end frame - always when Tb < L + (adjacent equal labels) - best_score is -inf and best_span (-1, -1).
 * threshold must lie in (-1e6, 0] (else LASR_E_ARG), so a dead state never passes it.  Starts are outputs only, never an index.
 * Emissions: where an utterance's rows fit LDS (C = 28; the predicate of the other lattice kernels, LASR_CTC_NO_LDS honoured)
 * they are staged once per workgroup with the exact row maxima; otherwise (C = 4334) a pre-pass writes the row maxima (B x T
 * f32) into the workspace and each lane gathers its class from global memory several frames ahead of the recursion.
 * Before any launch: a null pointer LASR_E_ARG; L_max outside [1, 64], K < 1, max_hits < 1, blank outside [0, C) or T * C >=
 * 2^31 LASR_E_SHAPE; a workspace below lasr_ctc_kws_workspace_bytes LASR_E_WORKSPACE. */
#define LASR_KWS_MAX_LABELS 64
size_t lasr_ctc_kws_workspace_bytes(int64_t B, int64_t T, int64_t K);
int lasr_ctc_kws(const float* logp, const int32_t* in_lens, int64_t B, int64_t T, int64_t C, int blank,
                 const int32_t* kw_labels, const int32_t* kw_offsets, int64_t K, int64_t L_max, float threshold, int max_hits,
                 int32_t* n_hits, int32_t* hit_span, float* hit_score, float* best_score, int32_t* best_span, void* workspace,
                 size_t workspace_bytes, void* stream);

/* Greedy CTC collapse of argmax ids (B, T) int32 truncated to lens (B) (NULL = T):
 * tokens (B, T) int32, n_tokens (B) int32.   utils/asr_metrics.py:159-166                      */
int lasr_greedy_decode(const int32_t* ids, const int32_t* lens, int64_t B, int64_t T, int blank,
                       int32_t* tokens, int32_t* n_tokens, void* stream);

/* Greedy CTC decode WITH confidences, straight from the log-probs: the collapsed tokens, their frame spans, per-token and
 * per-utterance confidences.  It replaces the host loop of the reference's pseudo-labelling (ssl_codec/utils.py:8-66, called
 * from train_ssl.py:223-260 on a (T', C) host copy per utterance): logp is read once, nothing larger than (B, T) is written.
 *
 * logp (B, T, C) f32 contiguous, entries finite or -inf (NaN is not supported); lens (B) int32, clamped to [0, T], NULL = T;
 * blank in [0, C).  For utterance b with Tb frames:
 *  - frame statistics: m_t = max_c logp[b][t][c] (exact), a_t = the lowest class attaining it - lasr_log_softmax's tie rule, so
 *    a tie between a label and the blank goes to the smaller id.  A row of -inf only has m_t = -inf, a_t = 0.  Frames t >= Tb
 *    are never read.
 *  - collapse (utils/asr_metrics.py:159-166; lasr_greedy_decode on a): frame t emits iff a_t != blank and (t == 0 or
 *    a_t != a_{t-1}).  Token i is the i-th emitting frame's class; its run is the maximal stretch of consecutive frames with
 *    that argmax, from the emitting frame on, cut at Tb.
 *  - per token, each (B, T): tokens = the class, -1 in slots i >= n_tokens[b]; tok_start / tok_end = the run's first frame and
 *    one past its last, -1 beyond n_tokens; tok_min = min of m_t over the run (exact), 0 beyond n_tokens; tok_mean = the f64
 *    sum of m_t over the run divided by the run length, rounded once to f32, 0 beyond n_tokens.
 *  - per utterance: n_tokens (B) int32; utt_sum (B, 2) f64: [0] = sum of m_t over t < Tb, [1] = the same over the frames with
 *    a_t != blank; n_nonblank (B) int32 = the number of those frames; conf (B, 2) f32:
 *        conf[k] = f32( -( -1e-5 + utt_sum[k] ) / ( n_k + 1e-6 ) ) evaluated in f64, n_0 = Tb, n_1 = n_nonblank.
 *    conf[0] is the reference's value: in sum_logprob / seq_sum_logprob_np the test `index == vocab_size` never fires (an
 *    argmax over C classes is at most C - 1), so blank frames are counted.  conf[1] is what that code evidently meant.
 *    Smaller is more confident (the reference's sign).  Tb == 0 gives 10.0; -inf propagates by IEEE rules.  The f64 sums are
 *    taken in an order of the kernel's choosing.
 * Two launches on `stream` (row statistics over the whole chip into the workspace, 8 * B * T bytes; then one workgroup per
 * utterance), nothing allocated or synchronised: the call can be captured in a hipGraph.  Refused before any launch: a null
 * pointer (lens excepted) LASR_E_ARG; blank outside [0, C), B * T >= 2^31, B < 1, T < 1 or C < 1 LASR_E_SHAPE (the workspace
 * function returns 0); a short workspace LASR_E_WORKSPACE.
 * lasr_greedy_confidence_frame_tile: the frames the collapse takes per step; lasr_greedy_confidence_narrow_classes: the
 * largest C whose rows share a wave in the row pass (wider rows take a wave each) - the sizes the tests put their cases at. */
int64_t lasr_greedy_confidence_frame_tile(void);
int64_t lasr_greedy_confidence_narrow_classes(void);
size_t lasr_greedy_confidence_workspace_bytes(int64_t B, int64_t T, int64_t C);
int lasr_greedy_confidence(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                           int32_t* tokens, int32_t* n_tokens, int32_t* tok_start, int32_t* tok_end,
                           float* tok_mean, float* tok_min, double* utt_sum, int32_t* n_nonblank, float* conf,
                           void* workspace, size_t workspace_bytes, void* stream);

/* CTC prefix beam search without an external scorer: beam_search.py:17-57 (ctc_decoders' ctc_beam_search_decoder_batch with
 * ext_scoring_func=None).  Per frame the classes ranked by (log-prob desc, id asc) are cut to the shortest leading run whose
 * cumulative probability reaches cutoff_prob (when < 1), then to cutoff_top_n; blank is pruned like any class.  Each prefix
 * keeps log_b / log_nb, score = logaddexp of the two; an extension p+c merges with a live prefix equal to it.  The beam_width
 * best entries survive, ties broken by (rank of the source prefix, "no new label" before a label, label id ascending).
 * Supported: beam_width 1..128, cutoff_top_n 1..64 (above C it acts as C), C <= 8192, any B and T with B*T and 1 + T*beam_width
 * below 2^31.  Outside that range the workspace function returns 0 and the decode LASR_E_SHAPE.  The workspace holds the
 * pruned frames (B*T*64 (class, log-prob)) and the prefix trie (B * (1 + T*beam_width) nodes of 8 bytes). */
size_t lasr_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t C, int beam_width, int cutoff_top_n);
/* logp (B, T, C) f32 log-probs (log_softmax output); lens (B) int32 frames per utterance (NULL = T; clamped to [0, T]).
 * tokens (B, n_best, T) int32: hypothesis j of utterance b in tokens[b][j][0 .. n_tokens[b][j]), -1 after it.
 * n_tokens (B, n_best) int32, scores (B, n_best) f32 = log-probability of the prefix, best first; slots past the number of
 * live prefixes hold n_tokens = -1 and score = -inf.  lens[b] = 0 gives the empty hypothesis with score 0.
 * LASR_E_ARG (nothing launched) for a null pointer, n_best outside [1, beam_width], cutoff_prob outside (0, 1] or blank outside
 * [0, C).  f32 arithmetic with a stable log-add; deterministic.  Two launches on `stream`, nothing allocated or synchronised. */
int lasr_ctc_beam_decode(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank, int beam_width,
                         int cutoff_top_n, float cutoff_prob, int n_best, int32_t* tokens, int32_t* n_tokens, float* scores,
                         void* workspace, size_t workspace_bytes, void* stream);

/* CTC prefix beam search fused with a character n-gram LM: beam_search.py:61-76 (BeamSearchDecoderWithLM with lm_path, i.e.
 * ctc_decoders' ctc_beam_search_decoder_batch with a character-based Scorer).  ctc_decoders' source is not part of this project;
 * what follows RESTATES its published behaviour (DESIGN.md "Beam search with an n-gram LM").  Everything above holds (pruning,
 * cutoff_prob / cutoff_top_n, log_b / log_nb, merging, tie-break); in addition:
 *  1. every label emission p -> p+c (c != blank; from score(p) when c != last(p), from log_b(p) when c == last(p)) adds
 *     alpha * lm(c | p) + beta.  The "no new label" continuation and blank add nothing, so the term depends on p+c alone.
 *  2. lm(c | p): the n-gram is the last N labels of p+c as strings (N = the ARPA's highest order), left-padded with <s> when
 *     p+c has fewer; scored by ARPA backoff (log10 p of the longest stored suffix ending in c, plus the log10 backoffs of the
 *     longer context suffixes, 0 for a context that is not stored), divided by NUM_FLT_LOGE = 0.4342944819.  If any word of the
 *     n-gram (padding included) is outside the LM's vocabulary (a label string the ARPA lacks, "<unk>", a missing <s>), the value
 *     is OOV_SCORE = -1000, unconverted.
 *  3. early cutoff: when the beam held beam_width prefixes after the previous frame, min_cutoff = score(last of them) +
 *     logp[t][blank] (unpruned) - max(0, beta); (p, c) contributes nothing where score(p) + logp[t][c] < min_cutoff (blank
 *     always passes).
 *  4. character-based LMs only (every ARPA word but <s>, </s>, <unk> is one code point), orders 1..6.
 *  5. hypotheses are ranked by the fused score (acoustic + the terms of 1); scores = fused, am_scores = ctc_decoders'
 *     approx_ctc = fused - labels * beta - alpha * sent_lm, sent_lm = the LM score of <s>^(N-1) labels </s> over N-word
 *     windows (<s>^N </s> for no labels).
 *
 * lasr_arpa_load reads a text ARPA file on the host (lightning_asr_amd/csrc/arpa_io.h) for the class strings vocab[0 .. n_vocab)
 * (UTF-8; class c uses vocab[c]; vocab may be NULL when n_vocab is 0) and returns a handle: LASR_E_ARG for a null pointer,
 * LASR_E_IO for a file that cannot be opened or read, LASR_E_FORMAT for a malformed file (the message names the line), an order outside 1..6, counts that disagree, a missing
 * suffix n-gram; LASR_E_UNSUPPORTED for a KenLM binary model.  lasr_arpa_info reports the order, whether the LM is
 * character-based, the n-grams kept (those over words some label maps to, and <s> / </s>) and the size of the device image;
 * lasr_arpa_write_image copies the image to host memory the caller then copies to the device (read-only, position-independent).
 * No device work and no device allocation. */
int lasr_arpa_load(const char* path, const char* const* vocab, int n_vocab, void** handle);
int lasr_arpa_info(const void* handle, int* order, int* char_based, int64_t* n_ngrams, size_t* image_bytes);
int lasr_arpa_write_image(const void* handle, void* host_dst, size_t bytes);
void lasr_arpa_free(void* handle);
/* The same workspace as lasr_ctc_beam_workspace_bytes. */
size_t lasr_ctc_beam_lm_workspace_bytes(int64_t B, int64_t T, int64_t C, int beam_width, int cutoff_top_n);
/* As lasr_ctc_beam_decode, with lm_image a device copy of a character-based image built for the vocabulary of classes
 * 0 .. C-1 (the blank's entry is never read).  scores = fused, am_scores = approx_ctc (-inf for an empty slot).  An image
 * whose header is not one lasr_arpa_write_image wrote yields empty slots (n_tokens -1) for every utterance.  LASR_E_ARG also
 * for a non-finite alpha or beta.  Two launches on `stream`, nothing allocated or synchronised; deterministic. */
int lasr_ctc_beam_decode_lm(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank, int beam_width,
                            int cutoff_top_n, float cutoff_prob, int n_best, const void* lm_image, float alpha, float beta,
                            int32_t* tokens, int32_t* n_tokens, float* scores, float* am_scores, void* workspace,
                            size_t workspace_bytes, void* stream);

/* CTC prefix beam search fused with a WORD-level n-gram LM and its lexicon (DESIGN.md "Beam search with a word-level LM").  It
 * restates ctc_decoders' word-based Scorer in this project's own words; ctc_decoders' source is not part of this project.
 * Everything of lasr_ctc_beam_decode holds (pruning, cutoff_prob / cutoff_top_n, log_b / log_nb, merging, tie-break).
 *  Mode.  An ARPA file is word-level when some word other than <s>, </s>, <unk> has more than one code point (lasr_arpa_info's
 *     char_based == 0).  It can be used when the vocabulary has exactly one label equal to " ": the space.
 *  Spellable words.  An LM word is spellable when every one of its code points is a one-code-point, non-space label.
 *     Unspellable words, <unk>, and every n-gram that contains one of them are left out of the image (the "drop unmapped
 *     words" rule, per word); <s> and </s> are kept.  The suffix-closure check runs on the file as read, before dropping.
 *  Lexicon.  A trie over the label ids of all spellable words; each prefix carries its trie node.  The empty prefix and a
 *     prefix that ends in the space sit at the root.  An extension by a non-space, non-blank label c exists only if the node
 *     has a child c; an extension by the space exists only if the node is a complete word - so no leading space, no double
 *     space, no out-of-lexicon word.  An extension that does not exist contributes nothing (-inf), like a candidate the early
 *     cutoff drops.  The trie state is reset at once on a space (ctc_decoders' one-frame delay after a word is not reproduced).
 *  Scoring.  A non-space label adds no LM term and no beta.  The space after word w adds alpha * lm(w | previous N-1 words,
 *     <s>-padded) + beta, lm as for lasr_ctc_beam_decode_lm: ARPA backoff in log10 divided by NUM_FLT_LOGE, OOV_SCORE = -1000
 *     unconverted if <s> is needed and the LM lacks it.  The term depends on the new prefix alone, so merging stays exact;
 *     beta is a per-word bonus.
 *  End of utterance.  A non-empty final prefix that does not end in a space gets one more term: alpha * lm(w | ...) + beta if
 *     its node is a complete word, alpha * OOV_SCORE + beta if it is not.  The <= beam_width final entries are then re-ranked
 *     by the new fused score, ties by their order before the term; n_best is cut from that order.
 *  Early cutoff.  As lasr_ctc_beam_decode_lm: min_cutoff = score(beam_width-th) + logp[t][blank] - max(0, beta) on a full
 *     beam, score the fused score without any end-of-utterance term.
 *  Outputs.  tokens / n_tokens as lasr_ctc_beam_decode_lm; scores = the fused score, end-of-utterance term included;
 *     am_scores = the acoustic logaddexp(log_b, log_nb), i.e. the fused score minus every term the search added.  This deviates
 *     from ctc_decoders' approx_ctc, which in word mode subtracts beta once per label while adding it once per word.
 *  Ranges.  Orders 1..6; beam width, cutoff_top_n, C, T, n_best and the workspace (lasr_ctc_beam_lm_workspace_bytes) as
 *     lasr_ctc_beam_decode_lm.
 *
 * lasr_arpa_load_words builds the word image (the n-gram sections of lasr_arpa_load over the spellable words, a lexicon behind
 * them, another magic: each search rejects the other kind of image) for vocab[0 .. n_vocab) with vocab[space_id] the only " ":
 * error codes and line-numbered messages as lasr_arpa_load, LASR_E_UNSUPPORTED also for a character-level file or a bad
 * space_id, LASR_E_FORMAT for a lexicon of more than 2^31 - 1 trie nodes.  lasr_arpa_info / _write_image / _free take its
 * handle; lasr_arpa_lexicon_info reports the spellable words, the trie nodes (the root included) and the words dropped as
 * unspellable (LASR_E_ARG for a handle of lasr_arpa_load). */
int lasr_arpa_load_words(const char* path, const char* const* vocab, int n_vocab, int space_id, void** handle);
int lasr_arpa_lexicon_info(const void* handle, int64_t* n_lexicon_words, int64_t* n_nodes, int64_t* n_dropped_words);
/* Arguments, checks and launches as lasr_ctc_beam_decode_lm, with lm_image a device copy of a word image.  Any other image
 * yields empty slots (n_tokens -1, scores -inf) for every utterance. */
int lasr_ctc_beam_decode_wlm(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank, int beam_width,
                             int cutoff_top_n, float cutoff_prob, int n_best, const void* lm_image, float alpha, float beta,
                             int32_t* tokens, int32_t* n_tokens, float* scores, float* am_scores, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Hotword biasing of the beam search (phrase boosting; DESIGN.md "Beam search with hotword biasing").  The caller hands over a
 * bank of phrases; the search favours hypotheses that spell them.  No LM is involved or retrained.
 *  Bank.  n_phrases phrases (0 is valid; at most 65 536), phrase i = labels[offsets[i] .. offsets[i+1]): 1..32 label ids in
 *     [0, C), none the blank; weights[i] finite and > 0, in natural-log units per matched label.  Duplicates are allowed.
 *  Automaton.  Over the trie of the phrases (at most 2^20 nodes, the root included) every node v carries depth(v); wmax(v), the
 *     largest weight of a phrase through v; credit(v) = depth(v) * wmax(v), evaluated in f64 and stored as f32 (root: 0);
 *     end(v): a phrase ends at v; leaf(v): end(v) and v has no child; keep(v): the credit of the deepest end node on the path
 *     root..v, v included (0 if none); fail(v): the node of the longest proper suffix of v's string that is a trie node (the
 *     root if none; fail(root) = root); max_credit: the largest credit of the bank (0 for an empty bank).
 *  step(v, c) -> (v', delta).  If v has a child u by c: delta = credit(u) - credit(v).  Otherwise w = fail(v); while w is not
 *     the root and has no child by c, w = fail(w); u = the child of w by c if it exists, else the root; delta = keep(v) -
 *     credit(v) + credit(u): the provisional credit beyond the last completed phrase is given back, the suffix match is
 *     credited.  v' = the root if leaf(u) (a completed phrase with no longer continuation is banked), else u.
 *  bonus(prefix) = the sum of the deltas over the prefix's labels from the root; state(prefix) = the node reached;
 *     final(prefix) = bonus(prefix) + keep(state) - credit(state): an unfinished match gives its provisional credit back at the
 *     end of the utterance.  All three are functions of the prefix alone.  Arithmetic is f32, one rounding per step; with
 *     weights that are multiples of 2^-k and small every value is exact.
 *  Image.  Read-only and position-independent: a 64-byte header (its own magic, n_nodes, max_credit, the table size, C and the
 *     blank), one 16-byte record per node (fail, credit, keep, flags) and an open-addressed hash (node, label) -> child, 16 bytes
 *     per slot at load <= 1/2.  No table over nodes x C exists.  lightning_asr_amd/csrc/hotword_io.h holds the builder, the
 *     layout and the one walker the host and the kernels both call.
 * lasr_hotword_build: LASR_E_ARG for a null pointer (labels / offsets / weights may be NULL only when n_phrases is 0), a
 * negative n_phrases, a blank outside [0, C), a label outside [0, C) or equal to the blank, an empty or over-long phrase or a
 * weight that is not finite and > 0; LASR_E_FORMAT for too many phrases or trie nodes.  The message names the phrase index.
 * lasr_hotword_info reports the phrases, the trie nodes (the root included), max_credit and the image size;
 * lasr_hotword_write_image copies the image to host memory (LASR_E_WORKSPACE when `bytes` is too small);
 * lasr_hotword_score is the host walk of labels[0 .. n) over the image: bonus, final and state of that prefix (any of the three
 * may be NULL; LASR_E_ARG for a label that is the blank or outside [0, C)).  None of them does device work. */
int lasr_hotword_build(const int32_t* labels, const int64_t* offsets /* n_phrases + 1 */, const float* weights, int n_phrases,
                       int64_t C, int blank, void** handle);
int lasr_hotword_info(const void* handle, int64_t* n_phrases, int64_t* n_nodes, float* max_credit, size_t* image_bytes);
int lasr_hotword_write_image(const void* handle, void* host_dst, size_t bytes);
void lasr_hotword_free(void* handle);
int lasr_hotword_score(const void* handle, const int32_t* labels, int64_t n, float* bonus, float* final_bonus, int32_t* state);
/* lasr_ctc_beam_decode with hotword biasing; bias_image is a device copy of a bank built for these C and blank.  Arguments,
 * checks, workspace (lasr_ctc_beam_workspace_bytes), prune launch and ranges as lasr_ctc_beam_decode, and everything stated
 * there holds (pruning, log_b / log_nb, merging, tie-break).  In addition:
 *  - the beam is ranked by logaddexp(log_b, log_nb) + bonus(p); log_b / log_nb stay acoustic;
 *  - an extension p -> p+c scores its acoustic value plus bonus(p) + delta(state(p), c); the "no new label" candidate keeps
 *    bonus(p); a p+c that merges into a live entry is that entry with its own bonus (the bonus depends on the prefix alone, so
 *    merging stays exact);
 *  - end of utterance: each final entry's bonus is replaced by final(p), the <= beam_width entries are re-ranked by the new
 *    score, ties by their order before, and n_best is cut from the new order.
 * scores = acoustic + final(p); am_scores = the acoustic logaddexp; bias_scores = final(p); all (B, n_best) f32.  An empty
 * slot holds -inf, -inf and 0.  An image whose header is not a hotword image for this C and blank yields empty slots
 * (n_tokens -1) for every utterance.  An image of 0 phrases reproduces lasr_ctc_beam_decode bit for bit in tokens, n_tokens
 * and scores.  LASR_E_ARG also for a null bias_image, am_scores or bias_scores.  Two launches on `stream`, nothing allocated
 * or synchronised; deterministic. */
int lasr_ctc_beam_decode_bias(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank, int beam_width,
                              int cutoff_top_n, float cutoff_prob, int n_best, const void* bias_image, int32_t* tokens,
                              int32_t* n_tokens, float* scores, float* am_scores, float* bias_scores, void* workspace,
                              size_t workspace_bytes, void* stream);
/* lasr_ctc_beam_decode_lm (character LM) with the same biasing: the emission term of its rule 1 becomes alpha * lm + beta +
 * delta; the early cutoff becomes min_cutoff = score(beam_width-th) + logp[t][blank] - max(0, beta) - max_credit, score the
 * fused score with bonus(p); end-of-utterance give-back and re-ranking as lasr_ctc_beam_decode_bias.  max_credit bounds what
 * one step can add wherever keep(v) <= credit(v), which holds unless a phrase outweighs a longer one it is a prefix of by more
 * than their lengths' ratio; the slack is part of the contract either way.  scores = the fused score with final(p) included;
 * am_scores = lasr_ctc_beam_decode_lm's approx_ctc, computed from the fused score without the bias; bias_scores = final(p).  A
 * wrong LM image or a wrong bias image yields empty slots.  An image of 0 phrases reproduces lasr_ctc_beam_decode_lm bit for
 * bit.  The word-level search (lasr_ctc_beam_decode_wlm) has no biased form: its lexicon already confines it to LM words. */
int lasr_ctc_beam_decode_lm_bias(const float* logp, const int32_t* lens, int64_t B, int64_t T, int64_t C, int blank,
                                 int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, const void* lm_image,
                                 float alpha, float beta, const void* bias_image, int32_t* tokens, int32_t* n_tokens,
                                 float* scores, float* am_scores, float* bias_scores, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* The resumable form of the five searches above: one sequence per stream, fed chunk by chunk.
 * CONTRACT: decoding a sequence in chunks of any sizes gives, after the last feed, the same tokens, n_tokens and f32 scores
 * (am_scores / bias_scores included) as the one-shot call of the same kind on the concatenated frames, bit for bit; and after
 * every feed the outputs are those of the one-shot call on the frames fed so far, end-of-utterance terms included (</s>, the
 * word LM's last word, the hotword give-back).  There is no finish call: the last feed's outputs are the result.
 *
 * The state lives in a caller-owned device buffer of lasr_ctc_beam_stream_state_bytes(B, T_cap, beam_width, kind): per stream
 * a 64-byte header (frames searched, live entries, which half of the beam is current, frames dropped, a live flag), an image
 * of the search kernel's LDS record for that kind (under 64 KB) and the prefix trie of 1 + T_cap * beam_width nodes.  The
 * buffer must be 16-byte aligned.  lasr_ctc_beam_stream_reset makes the streams listed in rows (DEVICE int32, n_rows of them;
 * NULL, 0: every stream; a row outside [0, B) is skipped) the empty prefix again: one launch, it reads no image, and it is also
 * how a fresh buffer is initialised.  B, T_cap, beam_width and kind describe the buffer and must be those of every feed.
 *
 * lasr_ctc_beam_stream_feed: logp (B, T_chunk, C) holds the next frames of each stream, lens (B) how many of them (NULL =
 * T_chunk, clamped to [0, T_chunk]; 0 = idle: the stream keeps its state and its outputs are rewritten).  scorer selects the
 * search and carries what that search takes beside the common arguments (unused fields are ignored); the images, alpha and
 * beta MUST NOT change between a reset and the last feed of a stream, nor may beam_width, cutoff_top_n, cutoff_prob, C or
 * blank: the saved state refers to them.  tokens (B, n_best, T_cap), n_tokens / scores (and scorer->am_scores / bias_scores)
 * (B, n_best) as in the one-shot calls; n_frames (B): frames searched so far; n_dropped (B): frames fed beyond T_cap, which are
 * counted and not searched (the device clamps; this is no error).  The workspace, lasr_ctc_beam_stream_workspace_bytes, holds
 * the kept lists of one chunk only.  A wrong LM or hotword image gives empty slots and leaves the state as it is.
 * Checks before any launch, as the one-shot calls: LASR_E_ARG for a null pointer (scorer, state, outputs, n_frames, n_dropped,
 * the images and score outputs the kind needs), an unknown kind, n_best outside [1, beam_width], cutoff_prob outside (0, 1],
 * blank outside [0, C), alpha / beta not finite; LASR_E_SHAPE outside the one-shot ranges for (B, T_chunk, C) or (B, T_cap)
 * (the size functions return 0 there); LASR_E_WORKSPACE for a state buffer or workspace too small.  A feed is two launches on
 * `stream`, nothing allocated or synchronised; it can be captured into a graph, and every replay advances the state. */
enum { LASR_BEAM_PLAIN = 0, LASR_BEAM_LM = 1, LASR_BEAM_WLM = 2, LASR_BEAM_BIAS = 3, LASR_BEAM_LM_BIAS = 4 };
typedef struct {
  int kind;                 /* LASR_BEAM_*: lasr_ctc_beam_decode, _lm, _wlm, _bias, _lm_bias */
  const void* lm_image;     /* LM, WLM, LM_BIAS */
  float alpha, beta;        /* LM, WLM, LM_BIAS */
  const void* bias_image;   /* BIAS, LM_BIAS */
  float* am_scores;         /* every kind but PLAIN */
  float* bias_scores;       /* BIAS, LM_BIAS */
} lasr_beam_scorer;
size_t lasr_ctc_beam_stream_state_bytes(int64_t B, int64_t T_cap, int beam_width, int kind);
size_t lasr_ctc_beam_stream_workspace_bytes(int64_t B, int64_t T_chunk, int64_t C, int beam_width, int cutoff_top_n);
int lasr_ctc_beam_stream_reset(void* state, size_t state_bytes, int64_t B, int64_t T_cap, int beam_width, int kind,
                               const int32_t* rows, int n_rows, void* stream);
int lasr_ctc_beam_stream_feed(const float* logp, const int32_t* lens, int64_t B, int64_t T_chunk, int64_t C, int blank,
                              int beam_width, int cutoff_top_n, float cutoff_prob, int n_best, const lasr_beam_scorer* scorer,
                              void* state, size_t state_bytes, int64_t T_cap, int32_t* tokens, int32_t* n_tokens, float* scores,
                              int32_t* n_frames, int32_t* n_dropped, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- optimiser ----------------
 * scheduler/novograd.py:75-145 with betas=(0.8,0.5), eps=1e-8, no amsgrad/grad_averaging/luc
 * (train.py:46), applied to all tensors in one pass over flat f32 buffers.
 * offsets (n_tensors+1) int64 element offsets into params/grads/exp_avg; exp_avg_sq (n_tensors) f32
 * (0 = "not initialised", scheduler/novograd.py:115).  lr is read from the device (1 f32) so a
 * captured graph can replay it.  grad_scale multiplies grads first (1/world after all-reduce).   */
size_t lasr_novograd_workspace_bytes(int64_t n_tensors, int64_t n_elems);
int lasr_novograd_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                       const int64_t* offsets, int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2,
                       float eps, float weight_decay, float grad_scale, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The same step for a caller that KEEPS its workspace: zero it once before the first call (the per-tensor norm accumulators live
 * there); every call leaves it zeroed, so the memset launch of lasr_novograd_step is not issued (round 5).                  */
int lasr_novograd_step_keep(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                            const int64_t* offsets, int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2,
                            float eps, float weight_decay, float grad_scale, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Weight EMA ("Weight EMA"): an exponential moving average of the PARAMETERS, kept in a flat f32 buffer `ema` of n_elems
 * and updated by the last kernel of the optimiser step, which holds the new parameters in registers: no launch is added.
 * Per element, three f32 operations of one rounding each (no FMA): diff = p_new - e; prod = w * diff; e = e + prod - bit-equal
 * to torch's `e + (p - e) * w`.  The weight comes from a device record (lasr_ema_state_bytes() bytes: int64 num_updates; float
 * decay; int warmup; float w): with t = num_updates, d = warmup ? min(decay, float(1 + t) / float(10 + t)) : decay (one correctly
 * rounded f32 division), w = 1.0f - d, then num_updates = t + 1 - computed by the step's moment kernel, so a captured graph
 * replays the warm-up and no host scalar enters the step.
 * lasr_ema_state_init: HOST only - fills a host image of the record for the caller to upload (like lasr_lr_schedule_init).
 *   LASR_E_ARG: a null or short buffer, decay outside [0, 1) or not finite, num_updates < 0.
 * lasr_novograd_step_ema: lasr_novograd_step (keep_workspace == 0) or lasr_novograd_step_keep (!= 0) with the average folded in.
 *   ema == NULL and ema_state == NULL: exactly the entry it mirrors, launch for launch and bit for bit.  LASR_E_ARG: one of
 *   the two without the other; ema overlapping params, grads or exp_avg.
 * lasr_ema_update: e[i] = e[i] + (p[i] - e[i]) * w over n elements with w from the host - the same expression outside a step
 *   (folding a parameter buffer into an average; the tests' yardstick).  A 4-byte head up to the first 16-byte boundary, 16-byte
 *   groups and a 4-byte tail (bases not congruent mod 16 bytes: 4-byte accesses throughout); one grid-strided launch of at most
 *   2048 workgroups, no workspace.  n == 0: returns 0, nothing launched.  LASR_E_ARG: a null pointer, n < 0, overlapping buffers. */
size_t lasr_ema_state_bytes(void);
int lasr_ema_state_init(void* host_buf, size_t bytes, float decay, int warmup, int64_t num_updates);
int lasr_novograd_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                           const int64_t* offsets, int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2,
                           float eps, float weight_decay, float grad_scale, void* workspace,
                           size_t workspace_bytes, void* stream, float* ema, void* ema_state, int keep_workspace);
int lasr_ema_update(float* ema, const float* params, int64_t n, float w, void* stream);

/* Gradient clipping and the non-finite-step guard ("Gradient clipping and the non-finite guard"), decided on the device inside
 * the optimiser step's own three launches.  One device record (lasr_clip_state_bytes() bytes: int64 steps; int64 skipped; int mode;
 * float clip_val; int skip_nonfinite; float total_norm; float coef; int last_skipped).  With s = grad_scale and g^ = s g (f32):
 *   mode 2 (value): g^ <- clamp(g^, -c, c) with torch's semantics (+-Inf -> +-c, NaN stays); the per-tensor norms and the update use it.
 *   mode 1 (norm):  N = (float)sqrt(sum_t norm2[t]) (f64, tensor index order), coef = min(1, c / (N + 1e-6f)) (one f32 add, one correctly
 *                   rounded f32 division); the update uses g^ coef, the per-tensor norm is coef^2 norm2[t].  coef == 1: every bit of the
 *                   step is the un-clipped step's.
 *   mode 0 (off):   the step as it is; the record is still filled in (total_norm: the global gradient norm, for logging).
 *   skip_nonfinite: when the sum of squares is not finite (any NaN or +-Inf; in value mode any NaN), the step writes nothing to params,
 *                   exp_avg, exp_avg_sq or ema and does not advance the EMA record; norm2 is re-zeroed; steps and skipped count it.
 *                   Off: a non-finite gradient behaves as without the record, and as torch (coef becomes NaN).
 * total_norm is the norm of the values the norm kernel squared: before the clip in norm mode, after the clamp in value mode.
 * lasr_clip_state_init: HOST only - fills a host image for the caller to upload.  LASR_E_ARG: a null or short buffer, a mode outside
 *   0..2, clip_val negative or not finite, a mode other than 0 with clip_val == 0, a negative count.
 * lasr_novograd_step_clip: lasr_novograd_step_ema with the record.  clip_state == NULL: that entry, launch for launch and bit for bit.
 *   With a record the moment kernel runs as ONE workgroup (the global norm needs every tensor's sum before any is re-zeroed). */
size_t lasr_clip_state_bytes(void);
int lasr_clip_state_init(void* host_buf, size_t bytes, int mode, float clip_val, int skip_nonfinite, int64_t steps, int64_t skipped);
int lasr_novograd_step_clip(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                            const int64_t* offsets, int64_t n_tensors, int64_t n_elems, const float* lr, float beta1, float beta2,
                            float eps, float weight_decay, float grad_scale, void* workspace,
                            size_t workspace_bytes, void* stream, float* ema, void* ema_state, int keep_workspace, void* clip_state);

/* Gradient accumulation (accumulate_grad_batches > 1; DESIGN 4, "Gradient accumulation"): acc[i] = acc[i] + g[i], a plain f32 add with one rounding
 * per element - bit-equal to `acc + g` in torch, whatever the alignment.  Every backward of the plan overwrites its whole
 * destination, so a window of K micro-batches backwards into a second flat buffer and adds it into the gradient the optimiser
 * reads; the 1/K average is the grad_scale of lasr_novograd_step.
 * lasr_grad_accumulate_ranges: [lo[i], hi[i]) are element offsets into BOTH buffers (host arrays, read before the call
 * returns), e.g. the pieces of one all-reduce bucket: one launch for all of them.  The pieces must not overlap; hi == lo is an
 * empty piece.  Each piece moves as a 4-byte head up to the first 16-byte boundary, 16-byte groups and a 4-byte tail; when
 * acc + lo and g + lo are not congruent mod 16 bytes the whole piece moves by 4-byte accesses, so no offset has to be a
 * multiple of 4.  One grid-strided launch of at most 2048 workgroups on `stream`; no workspace, no allocation, no
 * synchronisation.  n == 0 / no non-empty piece: returns 0, nothing launched.  LASR_E_ARG: a null pointer, n < 0, lo < 0,
 * lo > hi, n_ranges < 0 or above LASR_ACC_MAX_RANGES.  The buffers' lengths are the caller's to guard.                      */
#define LASR_ACC_MAX_RANGES 8
int lasr_grad_accumulate(float* acc, const float* g, int64_t n, void* stream);
int lasr_grad_accumulate_ranges(float* acc, const float* g, const int64_t* lo, const int64_t* hi, int n_ranges, void* stream);

/* roctx ranges (round 5; SURVEY 5 aux "tracing"): with LASR_ROCTX=1 in the environment the plan brackets its stages and units with
 * named ranges - "lasr:forward", "lasr:fwd <unit>", "lasr:head", "lasr:backward", "lasr:bwd <unit>", "lasr:wgrad flush", "lasr:reduce" -
 * through librocprofiler-sdk-roctx (dlopen'd on first use; a missing library switches the ranges off), so that
 * `rocprofv3 --marker-trace --kernel-trace` attributes kernels to units.  The host framework adds its own with the two calls below
 * (lightning_asr_amd/step.py: "lasr:step", "lasr:optimizer").  Host-side only: nothing is enqueued on any stream.                */
int lasr_roctx_range_push(const char* name);
int lasr_roctx_range_pop(void);
int lasr_roctx_enabled(void);

/* ---------------------------------------------------------------- measurement --------------
 * Optional per-kernel-class timing with HIP events recorded on the launch stream (bench.py's
 * roofline leg; off by default, costs two event records per instrumented launch when on).
 * lasr_prof_collect synchronises the recorded events and returns, per class: summed milliseconds,
 * summed algorithmic FLOPs and bytes (operands + result, each counted once) and launch count.     */
#define LASR_PROF_KINDS 5
enum { LASR_PROF_GEMM = 0,    /* every 1x1-conv GEMM launch (forward, data gradient, weight gradient, decoder) */
       LASR_PROF_DWCONV = 1,  /* depthwise conv forward / fused backward */
       LASR_PROF_BN = 2,      /* BatchNorm finalize + apply (+SE) forward, statistics + apply backward: one bracket per unit and direction */
       LASR_PROF_HEAD = 3,    /* log_softmax / CTC lattice + gradient (+ the next batch's features in its grid) / bias sums / loss mean */
       LASR_PROF_OTHER = 4 }; /* weight casts, length masks, deferred reductions, BiLSTM, column copies */
int lasr_prof_enable(int on);
int lasr_prof_collect(double* ms, double* flops, double* bytes, int64_t* count);
/* mean elapsed ms of n empty event pairs on `stream`: the bracketing overhead included in every ms[] entry */
int lasr_prof_overhead_ms(void* stream, int n, double* ms_per_pair);

/* Levenshtein distance between two token-id sequences, on the HOST (plain C++, no device work):
 * replaces editdistance.eval at utils/asr_metrics.py:54,220.  Returns -1 on bad arguments.       */
int64_t lasr_edit_distance(const int32_t* a, int64_t na, const int32_t* b, int64_t nb);

/* small helpers used by the plan and by the host */
int lasr_cast_f32_to_bf16(const float* in, void* out, int64_t n, void* stream);
/* out[r][0..cols) = bf16(in[r][:]), out[r][cols..ld_out) = 0: row-padded bf16 copy (ld_out % 8 == 0 keeps rows 16-byte aligned) */
int lasr_cast_pad_f32_to_bf16(const float* in, void* out, int64_t rows, int64_t cols, int64_t ld_out, void* stream);
size_t lasr_colsum_workspace_bytes(int64_t rows, int64_t C);
int lasr_colsum_f32(const float* x, float* out, int64_t rows, int64_t C, void* workspace, size_t workspace_bytes,
                    void* stream);                                   /* out[c] = sum_r x[r][c] (decoder bias grad) */
int lasr_scale_sum_f32(const float* x, int64_t n, float scale, float* out, void* stream); /* torch.mean, train.py:77 */

/* ---------------------------------------------------------------- whole model ---------------
 * MyModel2 (models/QuartNet.py:264-291; QuartNetContext.py:202; QuartNetContextSE.py:220) driven
 * as one native plan: the library sequences every kernel of forward, loss and backward on
 * `stream` from a single call, over caller-owned flat buffers.                                  */
typedef struct lasr_model lasr_model_t;

typedef struct {
  int32_t variant;   /* LASR_VARIANT_* */
  int32_t n_class;   /* len(labels)+1; blank = n_class-1 */
  int32_t in_c;      /* 64 */
  int32_t mask;      /* model.mask (conf/conf.yaml:36) */
  int32_t act;       /* LASR_ACT_RELU (reference) or LASR_ACT_SWISH */
  int32_t dtype;     /* activation dtype */
} lasr_model_config;

int lasr_model_create(const lasr_model_config* cfg, lasr_model_t** out);
void lasr_model_destroy(lasr_model_t* m);
/* One-shot feature prefetch: the next lasr_model_loss_backward[_partial] call on this model computes its CTC loss through
 * lasr_ctc_loss_mel with these lasr_mel_fwd arguments (channels-last output only), then forgets the request.  All
 * pointers are the caller's device buffers and must stay valid until that call has been enqueued. */
int lasr_model_set_prefetch(lasr_model_t* m, const float* wave, const int32_t* sample_lens, const float* dither,
                            const int32_t* aug, int64_t B, int64_t L, int normalize, void* out_btf, int dtype,
                            int32_t* frames_out, float* pct_out, void* mel_workspace, size_t mel_workspace_bytes);
/* the same with a lasr_wave_src (int16 PCM, dither generated on the device) */
int lasr_model_set_prefetch_src(lasr_model_t* m, const lasr_wave_src* src, const int32_t* sample_lens, const int32_t* aug,
                                int64_t B, int64_t L, int normalize, void* out_btf, int dtype, int32_t* frames_out,
                                float* pct_out, void* mel_workspace, size_t mel_workspace_bytes);
int lasr_model_clear_prefetch(lasr_model_t* m);   /* forget an armed request */
/* Tensors in reference state_dict order.  kind: 0 = parameter (lives in the flat param buffer at
 * `offset` elements), 1 = f32 buffer (running_mean/var, flat buffer array), 2 = num_batches_tracked
 * (int64, kept by the host).  Returns the number of tensors; fills row i when i >= 0.            */
/* nn.Dropout(p = drop_rate) of models/QuartNet.py:26,38,149 in every training forward / backward of this model (see
 * lasr_dropout above): step_counter is a caller-owned device scalar (uint64, zero-initialised); p = 0 switches it off.   */
int lasr_model_set_dropout(lasr_model_t* m, float p, uint64_t seed, uint64_t* step_counter);
int64_t lasr_model_tensor_info(const lasr_model_t* m, int64_t i, char* name, size_t name_cap,
                               int64_t shape[4], int32_t* ndim, int32_t* kind, int64_t* offset);
int64_t lasr_model_param_elems(const lasr_model_t* m);
int64_t lasr_model_buffer_elems(const lasr_model_t* m);
int64_t lasr_model_out_frames(const lasr_model_t* m, int64_t T_in);
size_t lasr_model_workspace_bytes(lasr_model_t* m, int64_t B, int64_t T_in, int64_t S_max);
/* Named intermediate ("tap": unit name, "<unit>.y", "<unit>.y2", "<unit>.u", "<unit>.se_hidden" (f32 [B][1][C/8]), "ctx_in", "logits", "grad_logits", "lens";
 * after a staged backward call "bwd.g_cur" = d(input of the last unit processed), "bwd.g_prev" = d(its output), both
 * [N][c] at the head of an [N][cmax] allocation) inside the workspace: returns its byte offset, or -1.            */
int64_t lasr_model_tap(lasr_model_t* m, const char* name, int64_t B, int64_t T_in, int64_t S_max, int64_t shape[3]);

/* feats: [B][T_in][in_c] channels-last in cfg.dtype (from lasr_mel_fwd / lasr_bct_to_btc).
 * logp_out (B, T', n_class) f32; argmax_out (B, T') int32 or NULL.  training=1 uses batch
 * statistics, updates `buffers`, and keeps what backward needs in the workspace.                */
int lasr_model_forward(lasr_model_t* m, const float* params, float* buffers, const void* feats,
                       const float* pct, int64_t B, int64_t T_in, int training, float* logp_out,
                       int32_t* argmax_out, void* workspace, size_t workspace_bytes, void* stream);
/* After a training forward in the same workspace: logp (B,T',C) as returned by it, grad_logp = dL/d logp
 * -> grads (flat f32, same layout as params; every element overwritten).                          */
int lasr_model_backward(lasr_model_t* m, const float* params, const void* feats, const float* logp,
                        const float* grad_logp, int64_t B, int64_t T_in, float* grads, void* workspace,
                        size_t workspace_bytes, void* stream);
/* forward + mean CTC (train.py:75-78) + backward in one call.  loss_out (1) f32, nll_out (B) f32. */
int lasr_model_loss_backward(lasr_model_t* m, const float* params, float* buffers, const void* feats,
                             const float* pct, const int64_t* targets, const int32_t* tgt_lens, int64_t B,
                             int64_t T_in, int64_t S_max, float* logp_out, float* loss_out, float* nll_out,
                             int32_t* argmax_out, float* grads, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Backward in stages, so the host can start the RCCL all-reduce of a gradient bucket while the units
 * below it are still being differentiated (Lightning DDP's bucketed overlap, conf/conf.yaml:30).
 * Units are numbered in forward order (lasr_model_unit_info gives their names).  _partial runs forward,
 * loss, the decoder and units [unit_stop, n); each _continue call runs units [unit_stop, previous stop).
 * Gradients of a unit's parameters are final once the call that covers the unit has been enqueued.
 * LASR_VARIANT_Q105: a residual block is five units, "<block>.seq.0" .. "<block>.seq.3" and the closing "<block>"; unit_stop may
 * fall inside a block (the residual branch's data gradient waits in the workspace for the block's first unit).       */
int64_t lasr_model_num_units(const lasr_model_t* m);
int lasr_model_unit_info(const lasr_model_t* m, int64_t i, char* name, size_t name_cap);
int lasr_model_loss_backward_partial(lasr_model_t* m, const float* params, float* buffers, const void* feats,
                                     const float* pct, const int64_t* targets, const int32_t* tgt_lens, int64_t B,
                                     int64_t T_in, int64_t S_max, float* logp_out, float* loss_out, float* nll_out,
                                     int32_t* argmax_out, float* grads, void* workspace, size_t workspace_bytes,
                                     int64_t unit_stop, void* stream);
int lasr_model_backward_continue(lasr_model_t* m, const float* params, const void* feats, int64_t B, int64_t T_in,
                                 float* grads, void* workspace, size_t workspace_bytes, int64_t unit_stop, void* stream);

/* ---- learning-rate schedule on the device -------------------------------------------------------------------------------
 * CosineAnnealingWarmupRestarts (scheduler/cosine_annearing_with_warmup.py:53-89; stepped per batch, train.py:57-61) as one
 * device-side state + a one-thread kernel: lasr_lr_schedule_init fills a HOST image of the state (the caller uploads it),
 * lasr_lr_schedule_step advances it and writes the rate lasr_novograd_step reads.  No host scalar enters a training step,
 * so the step can be captured into a hipGraph and replayed.                                                               */
size_t lasr_lr_schedule_state_bytes(void);
int lasr_lr_schedule_init(void* state_host_out, size_t bytes, int64_t first_cycle_steps, double cycle_mult, double max_lr,
                          double min_lr, int64_t warmup_steps, double gamma, int64_t cycle, int64_t step_in_cycle,
                          int64_t cur_cycle_steps, int64_t last_epoch);
int lasr_lr_schedule_step(void* state_dev, float* lr_dev, void* stream);

/* ---- large-vocabulary loss head (BASELINE cfg5: C = 4334): decoder 1x1 conv + log_softmax + CTC + their backward without the
 * (B, T', C) f32 log-prob / gradient tensors of models/QuartNet.py:275-290 and train.py:76-78 (444 MB each at bs = 32).
 * lasr_gemm_rowstat: C [M][ldc] bf16 = A [M][K] . B [N][K]^T + bias plus, per (row, 256-column tile), the softmax statistics
 *   of the STORED values: row_stat [M][tiles][2] = (max, sum exp(x - max)), row_arg [M][tiles] = first argmax column.
 * lasr_ctc_loss_lean: from those, lse and argmax per row, the lattice over the gathered target / blank emissions only, and
 *   grad [B*T][ldc] bf16 = gscale_b * d nll_b / d logits (1/B when gscale is NULL; zero rows past in_lens, NaN for an
 *   infeasible utterance like torch), bias_grad (C) f32 = column sums of the unrounded gradient.  ldc = C rounded up to 8.
 *   S_max <= LASR_CTC_MAX_LABELS; the workspace holds the lattice of lasr_ctc_workspace_bytes plus B*T*(S_max+1) f32
 *   emissions (0 above the bound). */
int lasr_gemm_rowstat(const void* A, const void* B, const float* bias, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                      float* row_stat, int32_t* row_arg, int* n_col_tiles, void* stream);
size_t lasr_gemm_rowstat_bytes(int64_t M, int64_t N);
size_t lasr_ctc_lean_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t S_max);
int lasr_ctc_loss_lean(const void* logits, int64_t ldc, const float* row_stat, const int32_t* row_arg, int n_col_tiles,
                       const int64_t* targets, const int32_t* in_lens, const int32_t* tgt_lens, int64_t B, int64_t T, int64_t C,
                       int64_t S_max, int blank, float* nll, int32_t* argmax, void* grad, float* bias_grad, const float* gscale,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Levenshtein distances of a batch ON THE DEVICE (utils/asr_metrics.py:26-59,187-228: editdistance.eval per utterance on
 * the host): hyp_tokens [B][ld_hyp] i32 / hyp_lens as written by lasr_greedy_decode, ref_tokens [B][ld_ref] i64 / ref_lens
 * as the collate's targets / target_sizes.  space_id < 0: units are token ids (CER; the reference's file-path
 * vocabularies); space_id >= 0: units are words = runs of tokens between space tokens (str.split()).
 * dist[b], ref_units[b] (B) i32; totals (may be NULL): totals[0] += sum dist, totals[1] += sum ref_units (the metric's
 * `scores` / `words` states).  At most 2048 tokens per utterance and side.                                               */
int lasr_edit_distance_batch(const int32_t* hyp_tokens, const int32_t* hyp_lens, int64_t ld_hyp, const int64_t* ref_tokens,
                             const int32_t* ref_lens, int64_t ld_ref, int64_t B, int space_id, int32_t* dist, int32_t* ref_units,
                             int64_t* totals, void* stream);

/* The alignment behind lasr_edit_distance_batch: which errors the distance is made of (what sclite, Kaldi's align-text and
 * jiwer print; the reference reports the total only).  Inputs, units (token ids, or words through the same 64-bit hash) and
 * limits are those of lasr_edit_distance_batch; dist / ref_units (B) i32 are bit-equal to what it writes.
 *   An alignment is a script of LASR_EDIT_HIT (a hypothesis unit paired with an equal reference unit), LASR_EDIT_SUB (paired
 *   with a different one), LASR_EDIT_DEL (a reference unit with no hypothesis unit), LASR_EDIT_INS (a hypothesis unit with no
 *   reference unit).  Several scripts of minimum cost usually exist and their counts differ ("a b" against "b a": two
 *   substitutions, or insertion + hit + deletion), so ONE is defined, in hypothesis / reference terms - not in terms of which
 *   side the kernel happens to lay along the wave: with D[i][j] the distance of the first i hypothesis units to the first j
 *   reference units, walk from (n_hyp, n_ref) back to (0, 0) and take at every cell the first that applies of
 *     1. diagonal:  i > 0, j > 0 and D[i-1][j-1] + (h_i != r_j) == D[i][j]   (a hit or a substitution),
 *     2. deletion:  j > 0 and D[i][j-1] + 1 == D[i][j],
 *     3. insertion: D[i-1][j] + 1 == D[i][j];
 *   the script is reported forwards, from the start of the utterance.
 * counts (B, 4) i32 = hits, substitutions, deletions, insertions; ops (B, ld_ops) u8 = the script, LASR_EDIT_PAD past n_ops[b];
 * n_ops (B) i32; ld_ops >= ld_hyp + ld_ref.
 * totals (may be NULL): i64[6] += sums of dist, ref_units, hits, substitutions, deletions, insertions.
 * confusion (may be NULL; token units only - LASR_E_ARG with space_id >= 0): (n_classes + 1) x (n_classes + 1) i32, += 1 at
 *   [reference label][hypothesis label] for every op, index n_classes standing for "none" (row n_classes: insertions, column
 *   n_classes: deletions, hits on the diagonal); an op with a token id outside [0, n_classes) is left out of the matrix.
 * workspace: lasr_edit_align_workspace_bytes = B * min(ld_hyp, ld_ref) * 64 * 8 (one 2-bit back-pointer per DP cell, a u64 per
 *   lane and DP row), rounded up to 256.  Nothing is allocated or synchronised; a refused call launches nothing.           */
enum { LASR_EDIT_HIT = 0, LASR_EDIT_SUB = 1, LASR_EDIT_DEL = 2, LASR_EDIT_INS = 3, LASR_EDIT_PAD = 255 };
size_t lasr_edit_align_workspace_bytes(int64_t B, int64_t ld_hyp, int64_t ld_ref);
int lasr_edit_align_batch(const int32_t* hyp_tokens, const int32_t* hyp_lens, int64_t ld_hyp, const int64_t* ref_tokens,
                          const int32_t* ref_lens, int64_t ld_ref, int64_t B, int space_id, int32_t* dist, int32_t* ref_units,
                          int32_t* counts, uint8_t* ops, int64_t ld_ops, int32_t* n_ops, int64_t* totals, int32_t* confusion,
                          int n_classes, void* workspace, size_t workspace_bytes, void* stream);

/* One training step's logged scalars (train.py:79-81: self.log('train_loss', loss) / self.log('train_wer', wer), on_step +
 * on_epoch) folded into DEVICE accumulators, so logging costs no D2H per step: with wer = sum(dist) / sum(ref_units) of the batch
 * (utils/asr_metrics.py:225-228; inf when the batch has no reference units),
 *   acc[0] += loss, acc[1] += wer, acc[2] += 1, acc[3] = loss, acc[4] = wer, acc[5] += sum(dist), acc[6] += sum(ref_units)
 * (7 doubles).  The host reads acc when it logs (every log_every_n_steps steps and at the end of the epoch).               */
int lasr_step_metrics(const float* loss, const int32_t* dist, const int32_t* ref_units, int64_t B, double* acc, void* stream);

/* ---- host ingest: wav files -> one int16 batch buffer -------------------------------------------------------------------
 * Replaces torchaudio.load in the reference's DataLoader workers (data_module.py:153; conf/conf.yaml:14 num_worker) and the
 * training-time random sub-sequence (data_module.py:138-148,158-159): n 16-bit PCM RIFF/WAVE files are decoded by up to
 * n_threads host threads straight into `out` (typically a pinned buffer) as rows of channel-0 samples,
 *   out[i][0 .. lens_out[i]) = the file's samples (or its crop), zeros up to the row pitch *ld_out = max length rounded up to 8,
 * ready for ONE H2D copy and lasr_mel_fwd_src(LASR_WAVE_PCM16).  crop_u (n, 2) doubles in [0,1) or NULL: per file,
 *   target = int(length * (crop_weight + (1 - crop_weight) * u0)); first = int(u1 * (length - target)); slice [first, target)
 * - the reference's sub_secquence, slice end included as it is there.  expect_rate > 0: fail on another sample rate.
 * No device work; returns LASR_E_WORKSPACE when n * ld exceeds out_capacity (elements).                                 */
int lasr_wav_info(const char* path, int64_t* n_frames, int32_t* n_channels, int32_t* sample_rate, int32_t* bits);
/* lead_in != 0: a crop that does not begin at the file's first sample is preceded in its row by the sample before it and its
 *   lens_out entry carries LASR_LEN_LEAD (see above: the reference crops AFTER pre-emphasis); the pitch counts the lead-in. */
int lasr_wav_read_batch(const char* const* paths, int64_t n, const double* crop_u, double crop_weight, int16_t* out,
                        int64_t out_capacity, int64_t* ld_out, int32_t* lens_out, int32_t expect_rate, int n_threads, int lead_in);

/* ---- sample-rate conversion: any-rate audio in, speed perturbation in training ---------------------------------------------
 * The reference feeds whatever rate torchaudio.load returns into a 16 kHz front-end (data_module.py:153 drops the rate); this is
 * the operator that was missing there: a polyphase Hann-windowed-sinc resampler (the interpolation torchaudio documents for
 * `resample` with its defaults, restated in DESIGN.md "Resampling"; torchaudio is not part of this project).
 * A conversion (sr_in, sr_out):  g = gcd; down = sr_in / g; up = sr_out / g; base = min(up, down) * rolloff;
 *   width = ceil(lpw * down / base); taps = 2 * width + down;
 *   h[p][k] = (base / down) * sinc(t) * cos(pi t / (2 lpw))^2,  t = clamp(((k - width) / down - p / up) * base, -lpw, lpw);
 *   n_out = ceil(n_in * up / down);  out[j] = sum_k h[j % up][k] * x[(j / up) * down + k - width],  x = 0 outside [0, n_in).
 * up == down == 1 is NOT run through the filter (which is no identity there): such a row is a plain copy.
 * Speed perturbation by s = a / b is the conversion (a, b): the clip becomes b / a as long, pitch moves with tempo (sox `speed`).
 *
 * The bank: up to 8 conversions as one position-independent image - a header table (up, down, width, taps, offset and the
 * kernel's tiling per conversion) followed by the taps, computed in f64, rounded once to f32, stored [tap][phase].  Built on the
 * host (lightning_asr_amd/csrc/resample.h), uploaded by the caller, read-only afterwards.  lpw = 6 and rolloff = 0.99 are the
 * defaults of the definition above.  LASR_E_ARG (lasr_resample_bank_bytes: 0) for a null list, n_conv outside [1, 8], a
 * non-positive rate, up or down above 1024, up * taps above 2^20, rolloff outside (0, 1], lpw outside [1, 64], a destination
 * smaller than the image.  No device work.
 * lasr_resample_out_len: ceil(n_in * up / down) for up, down in [1, 1024], n_in >= 0; -1 otherwise.
 * lasr_resample_tile: the outputs one workgroup of lasr_resample produces for the (reduced) conversion up / down - where its tests
 * put their row lengths; -1 for arguments no bank takes. */
size_t lasr_resample_bank_bytes(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff);
int lasr_resample_bank_write(const int32_t* sr_in, const int32_t* sr_out, int n_conv, int lpw, double rolloff, void* host_dst,
                             size_t bytes);
int64_t lasr_resample_out_len(int64_t n_in, int64_t up, int64_t down);
int64_t lasr_resample_tile(int64_t up, int64_t down, int lpw, double rolloff);
/* B rows in one launch on `stream`; nothing is allocated or synchronised, so the call can be captured.
 * bank_dev: a device copy of the image.  in: B rows of in_pitch elements, LASR_WAVE_F32 or LASR_WAVE_PCM16 (scaled by 1/32768,
 * exact); in_lens (B) int32 valid samples per row (required; clamped to in_pitch); conv_id (B) int32 = the row's conversion, NULL =
 * conversion 0 for every row.  out: B rows of out_pitch elements, f32 or PCM16 = clamp(rint(acc * 32768), -32768, 32767)
 * (saturating); f32 accumulation.  out_lens[b] = n_out; samples [n_out, L_out) of a row are written as zero, elements
 * [L_out, out_pitch) are not touched.  L_out must hold the longest row's n_out (a longer row is cut at L_out, out_lens says so).
 * An identity row (up == down == 1) is copied bit for bit when the dtypes agree, otherwise only the scale (and the rounding) apply;
 * its in_lens word passes through to out_lens, LASR_LEN_LEAD and the lead-in sample included.  On every other row a word carrying
 * LASR_LEN_LEAD is a CALLER ERROR (a filtered row has no lead-in sample: the flag is dropped and the lead-in sample is filtered as
 * the row's first sample).  A conv_id outside the bank, a bank without lasr_resample_bank_write's magic and count, or an entry whose
 * factors and tiling are outside the builder's limits gives a row of zeros with out_lens 0 (the taps themselves and the image's size
 * are the caller's: the call cannot know how long bank_dev is).  LASR_E_ARG: null pointer, unknown dtype, negative size, out_pitch < L_out; LASR_E_SHAPE: B > 65535, rows of
 * 2^31 samples or more. */
int lasr_resample(const void* bank_dev, const void* in, int in_dtype, int64_t in_pitch, const int32_t* in_lens,
                  const int32_t* conv_id, void* out, int out_dtype, int64_t out_pitch, int64_t L_out, int32_t* out_lens, int64_t B,
                  void* stream);

/* ---- waveform augmentation: reverberation with a room impulse response (RIR) and additive noise at a drawn SNR --------------
 * Row b has n valid samples x[0..n) (PCM16 scaled by 1/32768) and a parameter word (rir_id, noise_id, noise_start, snr_cdb), int32:
 * rir_id = -1: no reverb; noise_id = -1: no noise; snr_cdb = the SNR in hundredths of a dB.  (DESIGN.md "Noise and reverberation")
 *   reverb  y[j] = sum_{k < K} h[k] * x[j + d - k],  x = 0 outside [0, n), j in [0, n);  else y = x
 *   noise   v[j] = noise[off_c + (s + j) mod len_c]  for clip c = (off_c, len_c) and start s in [0, len_c);  else v = 0
 *   E_x = sum x^2, E_y = sum y^2, E_n = sum v^2 over [0, n) in f64;  g_s = sqrt(E_x / E_y) (1 without reverb, 0 if E_y == 0);
 *   g_n = sqrt(E_x / (E_n * 10^(snr_cdb / 1000))) (0 without noise or if E_x == 0 or E_n == 0)
 *   out[j] = g_s * y[j] + g_n * v[j] for j < n, 0 for j in [n, L);  out_lens[b] = n.  The length never changes.
 * f32 accumulation in ascending k, one fma per tap; the gains are formed in f64 and rounded once to f32; no float atomics: the
 * energies go through per-tile f64 partials in the workspace, summed in tile order, so a call gives the same bits every time.
 *
 * The RIR bank: up to 256 RIRs as one position-independent image - a header table (taps K, delay d, offset per RIR) followed by
 * the taps, unscaled f32 (lightning_asr_amd/csrc/wave_aug.h).  d = the first index of max |h|; K = the smallest length >= d + 1
 * whose dropped tail holds <= 1e-6 of the RIR's energy (f64), at most 8192.  rirs = the RIRs one after the other, lens[i] samples
 * each.  LASR_E_ARG (lasr_rir_bank_bytes: 0), naming the index: an empty RIR or one longer than 2^20 samples, an all-zero RIR,
 * a value that is not finite, d >= 8192, more than 256 RIRs, an image above 2^21 words, a destination smaller than the image.
 * No device work.
 * lasr_wave_augment_tile / _chunk: the outputs one workgroup of the FIR produces and the taps it stages per chunk - where the
 * tests put their row lengths and filter lengths.  lasr_wave_augment_workspace_bytes(B, L): 0 and LASR_E_SHAPE for B > 65535 or
 * L >= 2^31. */
size_t lasr_rir_bank_bytes(const float* rirs, const int64_t* lens, int n_rir);
int lasr_rir_bank_write(const float* rirs, const int64_t* lens, int n_rir, void* host_dst, size_t bytes);
int64_t lasr_wave_augment_tile(void);
int64_t lasr_wave_augment_chunk(void);
size_t lasr_wave_augment_workspace_bytes(int64_t B, int64_t L);
/* B rows on `stream` (three launches); nothing is allocated or synchronised, so the call can be captured.
 * rir_bank_dev: a device copy of the image, rir_bank_words its size in 4-byte words (NULL / 0: no RIRs).  noise_dev: the noise
 * bank, noise_total samples of noise_dtype (f32 or PCM16), clip c = noise_clips[2c] (offset), noise_clips[2c + 1] (length), int32
 * on the device (NULL / n_clips 0: no noise).  in: B rows of in_pitch elements; in_lens (B) int32 length words; params (B, 4) int32.
 * out: B rows of out_pitch elements, f32 (not clamped) or PCM16 = clamp(rint(v * 32768), -32768, 32767); elements [L, out_pitch)
 * are not touched.  `out` may be `in` itself (same pointer, dtype and pitch): the FIR writes y into the workspace and the mix
 * reads only that on reverberated rows.  out_lens (B) int32 (may be in_lens); stats (B, 3) f64 = (E_x, E_y, E_n) (E_y = E_x
 * without reverb).  workspace: lasr_wave_augment_workspace_bytes(B, L) bytes on the device, 16-byte aligned.
 * A row with rir_id == noise_id == -1 is copied bit for bit when the dtypes agree (otherwise only the scale and the rounding
 * apply); its length word passes through, LASR_LEN_LEAD and the lead-in sample included.  On every other row the flag is masked:
 * an augmented row has no lead-in sample (a CALLER ERROR, refused by the Python wrappers).  An id outside its bank, a clip that
 * runs past noise_total, a start outside [0, len_c), a bank without lasr_rir_bank_write's magic, or an entry outside the builder's
 * limits or past rir_bank_words gives a row of zeros with out_lens 0; nothing is read out of bounds.  LASR_E_ARG: null pointer,
 * unknown dtype, negative size, a pitch below L, a partial alias of in and out, a small or misaligned workspace; LASR_E_SHAPE:
 * B > 65535, rows of 2^31 samples or more. */
int lasr_wave_augment(const void* rir_bank_dev, int64_t rir_bank_words, const void* noise_dev, int noise_dtype,
                      const int32_t* noise_clips, int n_clips, int64_t noise_total, const void* in, int in_dtype, int64_t in_pitch,
                      const int32_t* in_lens, const int32_t* params, void* out, int out_dtype, int64_t out_pitch, int64_t L,
                      int32_t* out_lens, double* stats, int64_t B, void* workspace, size_t workspace_bytes, void* stream);

/* ---- long recordings: voice-activity segmentation and the gather from segments to batch rows ---------------------------------
 * One recording is one row.  Everything after the quantisation of a sample is integer arithmetic, so the result is exact in any
 * summation order (DESIGN.md "Inference: long recordings"; lightning_asr_amd/csrc/segment.h has the host side):
 *   q = the PCM16 sample, or clamp(rint(x * 32768), -32768, 32767) (half to even) of an f32 one
 *   frame n = samples [160 n, 160 n + 160) of the row's len samples, F = ceil(len / 160);  E[n] = sum q^2 (64-bit)
 *   lev[n] = 0 for E == 0, else 8 k + m + 1, k = floor(log2 E), m = the three bits of E below its leading one (0.376 dB a step)
 *   floor = the max(1, ceil(F * floor_permille / 1000))-th smallest level;  base = min(max(floor, min_level), max_floor_level)
 *   on = base + on_steps, off = base + off_steps;  a maximal run of lev >= off is speech iff one of its frames has lev >= on
 *   close: a run that starts fewer than min_silence frames after the previous kept run's end is merged into it
 *   open:  runs shorter than min_speech frames are then dropped
 *   pad:   [max(0, s - pad), min(F, e + pad)); a run whose padded start is <= the previous padded end merges with it
 *   split: while e - s > max_frames, cut at the first frame of lowest level in [s + max_frames / 2, s + max_frames)
 *   segment = samples [160 s, min(160 e, len)), in time order.
 * lasr_vad_params_from fills the struct from dB and seconds: steps = round(dB / (10 log10(2) / 8)); an absolute level = the level
 * of round(160 * 32768^2 * 10^(dBFS / 10)); frames = round(seconds * 100), all half to even.  LASR_E_ARG: a value that is not
 * finite, |dB| > 1000, a level above 0 dBFS, seconds outside [0, 1e6], and what lasr_vad_segment checks too: 0 <= off_steps <=
 * on_steps, floor_permille in 1..1000, 0 <= min_level <= max_floor_level < LASR_VAD_LEVELS, max_frames >= 2, frame counts in [0, 2^30].
 * lasr_vad_sweep: the frames (and runs) one workgroup takes per sweep of its passes - where the tests put their row lengths.
 * lasr_vad_workspace_bytes(B, L): 0 and LASR_E_SHAPE for B > 65535 or L >= 2^31. */
#define LASR_VAD_LEVELS 512
typedef struct {
  int32_t on_steps, off_steps, floor_permille, min_level, max_floor_level, min_silence, min_speech, pad, max_frames;
} lasr_vad_params;
int lasr_vad_params_from(double on_db, double off_db, int floor_permille, double min_level_db, double max_floor_db,
                         double min_silence_s, double min_speech_s, double pad_s, double max_segment_s, lasr_vad_params* out);
int64_t lasr_vad_sweep(void);
size_t lasr_vad_workspace_bytes(int64_t B, int64_t L);
/* B rows on `stream` (a memset and two launches); nothing is allocated or synchronised, so the call can be captured.
 * wave: B rows of `pitch` elements (0 = L), LASR_WAVE_F32 or LASR_WAVE_PCM16; sample_lens (B) int32 plain sample counts, clamped to
 * [0, L] (NULL = L).  segs (B, max_segments, 2) int32 = (start, end) in samples; n_segs (B) int32 = the TRUE count - when it exceeds
 * max_segments only the first max_segments are written and the caller decides whether that is an error; rows of segs past the
 * count are not touched.  floor_out (B) int32 = the noise floor level before its clamps (0 for an empty row), may be NULL.
 * levels_out (B, ceil(L / 160)) uint16 = lev, 0 past a row's F, may be NULL (tests and diagnosis).  workspace:
 * lasr_vad_workspace_bytes(B, L) bytes on the device, 16-byte aligned. */
int lasr_vad_segment(const void* wave, int wave_dtype, int64_t pitch, const int32_t* sample_lens, int64_t B, int64_t L,
                     const lasr_vad_params* params, int32_t* segs, int64_t max_segments, int32_t* n_segs, int32_t* floor_out,
                     uint16_t* levels_out, void* workspace, size_t workspace_bytes, void* stream);
/* table: (n, 3) int32 (row, start, end) in HOST memory, read before the call returns (up to 256 entries travel in the arguments of
 * one launch).  out (n, out_pitch) in the input's dtype on the device: row i = samples [start, end) of source row `row` (rows of
 * `pitch` elements), then zeros up to out_pitch; out_lens[i] = end - start.  The caller answers for row and end lying inside
 * `wave`.  LASR_E_ARG: null pointer, row < 0, start < 0, end < start; LASR_E_SHAPE: a segment longer than out_pitch. */
int lasr_segment_gather(const void* wave, int wave_dtype, int64_t pitch, const int32_t* table, int64_t n, void* out,
                        int64_t out_pitch, int32_t* out_lens, void* stream);

/* ---- data-parallel gradient exchange: RCCL over xGMI, called by the library itself ------------------------------
 * Replaces the NCCL all-reduce the reference gets from Lightning's DDP plugin (conf/conf.yaml:30-31 `accelerator: ddp`,
 * train.py:239): SUM over ranks of the flat f32 gradient, bucket by bucket while backward is still
 * running, plus the wrap-time broadcast of parameters and buffers from rank 0.
 * One communicator per process (one process per GPU).  Collectives run on a library-owned side stream:
 *   lasr_comm_allreduce / _ranges / lasr_comm_broadcast   wait (event) for everything enqueued on `producer_stream` so far,
 *                                                         then run in place on the side stream;
 *   lasr_comm_wait                                        makes `consumer_stream` wait for every collective issued so far.
 * No call synchronises the host.  Positive return codes 1000+n carry ncclResult_t n.
 * Bootstrap: rank 0 calls lasr_comm_unique_id and the host carries the LASR_COMM_ID_BYTES bytes to the other ranks by
 * whatever rendez-vous it has (torch.distributed's store, MPI, a file); every rank then calls lasr_comm_init.        */
#define LASR_COMM_ID_BYTES 128
typedef struct lasr_comm lasr_comm_t;
int lasr_comm_unique_id(void* id_out, size_t id_bytes);
int lasr_comm_init(lasr_comm_t** out, const void* unique_id, size_t id_bytes, int world, int rank, int device);
int lasr_comm_destroy(lasr_comm_t* comm);
int lasr_comm_world(const lasr_comm_t* comm);
int lasr_comm_rank(const lasr_comm_t* comm);
int lasr_comm_allreduce(lasr_comm_t* comm, float* buf, int64_t count, void* producer_stream);
/* one bucket made of several pieces of the flat buffer (ncclGroupStart/End: one fused launch) */
int lasr_comm_allreduce_ranges(lasr_comm_t* comm, float* base, const int64_t* lo, const int64_t* hi, int n_ranges,
                               void* producer_stream);
int lasr_comm_broadcast(lasr_comm_t* comm, float* buf, int64_t count, int root, void* producer_stream);
int lasr_comm_wait(lasr_comm_t* comm, void* consumer_stream);
/* LASR_COMM_MAX_CHANNELS=n (> 0) makes lasr_comm_init set NCCL_MAX_NCHANNELS=n (the persistent workgroups a collective keeps resident
 * on the CUs it shares with the backward) unless that variable is already set; default 0 = RCCL's own choice (measured: the
 * interference grows with the LENGTH of the exchange, not with the CUs it holds - DESIGN 5).
 * Timing of the exchange (bench.py's `comm` record; eager launches only): with timing on, every collective is bracketed by events on
 * the side stream and every lasr_comm_wait by events on the consumer stream.  lasr_comm_timing_collect synchronises them and returns,
 * in call order, coll_us[i] / coll_bytes[i] (duration and payload of collective i, peers' arrival included) and wait_us[j] (how long
 * consumer stream j-th wait actually stalled: the part of the exchange backward did not hide); at most max_recs entries are written,
 * *n_coll / *n_waits are the numbers recorded since timing was switched on.                                                      */
int lasr_comm_timing(lasr_comm_t* comm, int on);
int lasr_comm_timing_collect(lasr_comm_t* comm, int max_recs, double* coll_us, double* coll_bytes, int* n_coll, double* wait_us,
                             int* n_waits);

#ifdef __cplusplus
}
#endif
#endif /* LASR_H */
