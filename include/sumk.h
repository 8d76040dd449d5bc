/* sumk.h -- C ABI of libsumk.so: MI355X (gfx950) frame-importance scoring kernels.
 *
 * Drop-in boundary for the sequence-scorer hot path of sylvainma/Summarizer.  The reference has NO native
 * layer: its hot path is the implicit ATen dispatch under the nn.Module.forward calls
 * cited per entry point below, so each entry replaces "what torch would run" for one reference call site.
 * Python binds this header with ctypes (summarizer_amd/_lib.py); a maintainer's stub is in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; sumk_last_error() gives the message (thread local).
 *  - all matrices are dense row-major fp32 in DEVICE memory, BORROWED for the duration of the call.
 *  - a batch of videos is PACKED: frames of video s are rows [seq_off[s], seq_off[s+1]) of every per-frame
 *    matrix.  seq_off is given twice: a host copy (grid sizing, workspace carving) and a device copy
 *    (read by the kernels).  n_rows == seq_off[n_seq].
 *  - no hidden allocation: the caller owns the workspace; query its size first.
 *  - `stream` is a hipStream_t (passed as void*); calls only enqueue work and are graph-capturable.
 *  - D (feature size) and H (LSTM hidden size) must be multiples of 4.
 */
#ifndef SUMK_H
#define SUMK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SUMK_OK 0
#define SUMK_ERR_ARG (-1)       /* bad shape / null pointer / unsupported size */
#define SUMK_ERR_WORKSPACE (-2) /* workspace too small */
#define SUMK_ERR_HIP (-3)       /* HIP runtime error (message has hipGetErrorString) */

const char* sumk_last_error(void);
int sumk_version(void);
/* number of HIP devices visible; <0 if the runtime cannot be initialised (the library never falls back to CPU) */
int sumk_device_count(void);

/* GEMM arithmetic selectors (see sumk_vasnet_opts.precision) */
#define SUMK_PRECISION_FP32 0
#define SUMK_PRECISION_BF16X3 1
#define SUMK_PRECISION_BF16X6 2   /* x = x1+x2+x3 exactly, 6 bf16 MFMAs per product: fp32-grade results */
#define SUMK_PRECISION_BF16 3     /* plain bf16 operands (one plane), ONE bf16 MFMA per product, fp32 accumulate: the mixed-precision
                                     TRAINING arithmetic of BASELINE config 2 (storage, master weights and optimiser stay fp32) */
#define SUMK_PRECISION_MAX 3

/* ------------------------------------------------------------------------------------------------ VASNet
 * Weights of summarizer/models/vasnet.py:56-66, each as stored by nn.Linear ([out][in]).
 * The SAME layer_norm (ln_w, ln_b) is applied twice (vasnet.py:137 and :143). */
typedef struct sumk_vasnet_weights {
  const float* Wk; const float* Wq; const float* Wv; /* (D,D)  K/Q/V.weight            vasnet.py:57-59 */
  const float* Wo;                                   /* (D,D)  attention_head_projection vasnet.py:60  */
  const float* W1; const float* b1;                  /* (D,D),(D)  k1                   vasnet.py:64   */
  const float* w2; const float* b2;                  /* (D),(1)    k2                   vasnet.py:65   */
  const float* ln_w; const float* ln_b;              /* (D)        layer_norm           vasnet.py:54   */
} sumk_vasnet_weights;

typedef struct sumk_vasnet_opts {
  float scale;          /* logits multiplier, 1/sqrt(D) by default      vasnet.py:34,119 */
  float eps;            /* LayerNorm epsilon                            vasnet.py:18,54  */
  int32_t ignore_self;  /* diag -> -inf                                 vasnet.py:121-122 */
  int32_t aperture;     /* -1 = global; w>=0: |i-j|>w -> -inf, and in-band logits with e*e==0 -> -inf
                           (tril*triu==0 quirk)                         vasnet.py:124-127 */
  /* training-mode dropout (vasnet.py:53,130,136,142): p=0 disables (eval).  Keep-masks are a pure function
     of (seed, site, element index) -- see DESIGN.md "Dropout" -- so backward regenerates them. */
  float dropout_p;
  uint64_t seed;
  /* arithmetic of the GEMMs: SUMK_PRECISION_FP32 (native fp32 MFMA, the default everywhere), SUMK_PRECISION_BF16X6 (operands
     split exactly into three bf16 planes, 6 bf16 MFMAs per product: fp32-grade results, DESIGN.md "bf16x6") or
     SUMK_PRECISION_BF16X3 (fp32 operands split into bf16 hi+lo, 3 bf16 MFMAs per product, fp32 accumulate: ~2^-16 relative
     per product, scores stay within ~1e-5 of the fp32 path -- DESIGN.md "bf16x3").  Storage is fp32 either way. */
  int32_t precision;
  /* NULL, or a device word the kernels ADD to `seed` when they run: the masks of a call are then a function of (seed + *seed_dev),
     read at execution time.  For steps captured into a HIP graph: kernel arguments are frozen at capture, the device word is not --
     the caller increments it between replays (after the backward pass of a step) and every replay draws fresh masks. */
  const uint64_t* seed_dev;
  /* NULL, or the batch's problem tables prebuilt by sumk_vasnet_build_tables for the SAME (D, seq_off, training, precision): the call
     then launches no table-setup kernel (5-7 us per call: 5 % of a single-video forward).  The tables depend on the batch geometry
     only -- not on weights, inputs or the workspace -- so a caller builds them once per distinct batch (SeqBatch in kernels.py) and
     may share them between forward, backward and any number of calls ON ONE STREAM AT A TIME (they hold the tickets of the
     in-launch split-K launches, which every launch leaves zero).  Wrong tables give wrong results, not errors: device memory. */
  void* tables;
  /* NULL, or bf16(x) (n_rows, D) written by sumk_cast_f32_bf16 from the SAME x this call (forward and backward) is given: the mixed-precision
     training step (training != 0, SUMK_PRECISION_BF16 on the bf16-source kernels) then reads it instead of casting x again -- features
     are constant over the epochs of a run while the weights change every step, and x is 70 % of the elements the per-step cast kernel
     converts.  Ignored by every other mode.  Not allowed together with pos_table (which changes x in place). */
  const void* x16;
  /* NULL, or -- for inference in SUMK_PRECISION_BF16X6 / BF16X3 -- the "KB planes" (below) of the SAME x (n_rows x D; 3 resp. 2 planes)
     written by sumk_split_planes, and the weight-plane block written by sumk_vasnet_wplanes_build for the SAME weights and plane count.
     With both given (and D % 256 == 0, n_rows >= 256, no pos_table) the three row-wise GEMMs of the call -- K/Q/V projection, output
     projection, k1 (vasnet.py:114-116,132,138) -- run on the plane-aware wide kernel (csrc/gemm_pw.hip): no fp32 -> bf16 split inside any
     k-loop.  Same arithmetic as without them (the planes are the roundings the in-loop kernels make), faster.  x planes are constant per
     dataset, weight planes per weight change; stale planes give wrong results, not errors.  The per-video products follow: T <= 320 on the
     plane strips (csrc/attn_pw.hip), every video of the batch with T >= 1536 (round 6) as launches of the plane GEMM itself -- both need the
     larger workspace sumk_vasnet_workspace_bytes_for reports for the precision; anything else keeps the in-loop kernels between plane GEMMs. */
  const void* xplanes;
  const void* wplanes;
} sumk_vasnet_opts;


/* Bytes of workspace sumk_vasnet_forward / _backward need for this batch (seq_off_host has n_seq+1 entries). */
size_t sumk_vasnet_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t training);
/* The same for a known arithmetic: only the mixed-precision training step (training != 0, SUMK_PRECISION_BF16) needs the bf16
 * operand shadows at the end of the workspace (~ +25 %); every other mode is content with this smaller size.  Which kernels a step
 * runs on never depends on the workspace it is handed: a bf16 training step given the smaller workspace is refused
 * (SUMK_ERR_WORKSPACE), so a forward and a backward pass cannot end up on different paths. */
size_t sumk_vasnet_workspace_bytes_for(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t training, int32_t precision);

/* ------------------------------------------------------------------------------------------------ local attention on the band (long videos)
 * VASNet's `local` option (sumk_vasnet_opts::aperture = w >= 0, vasnet.py:124-127) for videos the dense path cannot hold: there the logits
 * are a full (T x T) block per video with the mask applied afterwards, so workspace and FLOPs grow with T^2 whatever w is
 * (csrc/attn_band.hip).  Here, per video of a packed batch, ctx = softmax(mask(Q K^T * scale)) V over the keys [i - w, i + w] of every
 * query row i only.  The definition -- scale, ignore_self, the tril * triu == 0 rule that also masks in-band logits whose square is 0, NaN
 * for a row with every key masked -- is that of the dense path.  What differs:
 *   storage  a video is cut into strips of 64 query rows; strip r keeps a rectangle of 64 x (k_hi - k_lo) fp32 logits for the keys
 *            k_lo = max(0, 64 r - w) .. k_hi = min(T, 64 r + 64 + w), pitch = min(T, 2 w + 64) rounded up to 4, all strips of all videos
 *            back to back, every offset 64-bit: the workspace is O(T w), nothing of size T x T exists;
 *   launches one setup launch, then three: the logits of every strip (ONE grouped exact-fp32 NT launch, a problem per strip, the kernel and
 *            k order of the dense path's per-video launch), the band softmax in place (one wave per row), the context of every strip
 *            (ONE grouped NN launch contracting over exactly the strip's k_hi - k_lo keys: V rows of the next video, or scratch behind
 *            the last one, are never multiplied -- 0 x NaN would be NaN).  No atomics, no cooperative launch, no flag polled across
 *            workgroups; bit-deterministic; only enqueues work (captures into a HIP graph).
 * sumk_attn_band: Q, K, V (rows x D, leading dimensions ldq / ldk / ldv) -> ctx (rows x D, ldc).  alpha: NULL, or (rows x (2 w + 1)) floats
 * that receive the attention weights, entry c of row i = key i - w + c, zeros for keys outside the video (a test entry; w <= 1048576).
 * sumk_vasnet_forward_band: inference of vasnet.py:114-145 with steps 118-131 on the band -- QKV projection, the launches above, output
 * projection + residual, LayerNorm, k1 + ReLU, LayerNorm + k2 + sigmoid.  x is NOT modified (a caller with positions adds them beforehand);
 * opts->tables / x16 / xplanes / wplanes are ignored.
 * Limits: aperture >= 0 (any value: the key range is clipped to the video), D % 4 == 0, 1 <= T <= 1048576 per video, at most 65535
 * videos, leading dimensions >= D and % 4 == 0; the forward also needs opts->precision == SUMK_PRECISION_FP32 and dropout_p == 0.
 * Anything else returns SUMK_ERR_ARG (a short workspace: SUMK_ERR_WORKSPACE), sets sumk_last_error and launches nothing.
 * The *_workspace_bytes functions are pure host arithmetic (0 = bad arguments): about 4 T (2 w + 64) bytes per video for the band, plus
 * 20 T D bytes of activations for the forward. */
size_t sumk_attn_band_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture);
int sumk_attn_band(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D, int32_t n_seq,
                   const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale, int32_t ignore_self, int32_t aperture, float* ctx,
                   int32_t ldc, float* alpha, void* workspace, size_t workspace_bytes, void* stream);
size_t sumk_vasnet_band_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture);
int sumk_vasnet_forward_band(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                             const sumk_vasnet_weights* w, const sumk_vasnet_opts* opts, float* scores, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ TRAINING on the band
 * The attention above with what its backward needs kept, and that backward, in O(T w) per video (csrc/attn_band_bwd.hip).  A training
 * workspace holds THREE rectangle buffers of the scoring layout: E (alpha), E2 (dropout(alpha) forward; dAlphaD, then dLogits, backward) and
 * ET (transposed rectangles).  The band is symmetric -- key strip c is seen by exactly the query rows ab_k_lo(w, c) .. ab_k_hi(T, w, c), the
 * count, pitch and offset of strip c's own rectangle -- so with a rectangle transposed into ET, dV = alphaD^T dCTX and dK = dLogits^T Q are the
 * scoring path's context launch again: ONE grouped NN launch, a problem per key strip contracting over exactly its query rows.
 * Backward launches, given dCTX: setup; transpose(alphaD); dV; dAlphaD = dCTX V^T (the logits launch); softmax backward in place
 * (dLogits = scale * alpha * (drop'(dAlphaD) - sum_j drop'(dAlphaD)_j alpha_j)); dQ = dLogits K; transpose(dLogits); dK.  No atomics, no
 * cooperative launch, no flag polled across workgroups; bit-deterministic; every call only enqueues work (captures into a HIP graph).
 * Dropout of alpha (site 0) draws entry (packed row r, key j of the video) at index (r << 20) | j -- the dense path's index, so one seed
 * gives a dense and a band model the same masks; the 20 key bits are exactly the limit of 1048576 steps.  seed_dev: NULL, or a device word
 * the kernels add to `seed` when they run (sumk_vasnet_opts::seed_dev).
 * NaN: an all-masked query row i has NaN weights; its dQ row is NaN and NaN reaches dK / dV only at the keys [i - w, i + w] (the dense path
 * spreads it over the whole video).  A NaN video never reaches another video's gradients.
 * sumk_attn_band_forward_train: as sumk_attn_band (no alpha output), leaving alpha / dropout(alpha) in the workspace.
 * sumk_attn_band_backward: reads the workspace the forward left (same batch, aperture, dropout_p and seed) -> dQ, dK, dV (rows x D).
 * sumk_vasnet_forward_band_train: vasnet.py:114-145 in training mode -- the three dropout sites, sites 1 and 2 (before either LayerNorm)
 * indexed as the dense path -- keeping [Q | K | V], the context, both LayerNorm inputs, their statistics and the scores in the workspace.
 * sumk_vasnet_backward_band: the stage order of sumk_vasnet_backward's large-batch path; weight gradients ACCUMULATE into `grads`;
 * dx (NULL, or rows x D) = dY0 + dQ Wq + dK Wk + dV Wv; tail_grads_ready_event (NULL, or a hipEvent_t) is recorded once the gradients of
 * Wo, W1, b1, w2, b2 are final.  x is NOT modified; opts->tables / x16 / xplanes / wplanes are ignored.
 * Limits and status codes are those of the band forward; exact fp32 only; 0 <= dropout_p < 1; the VASNet pair also needs D <= 2048.
 * A short workspace returns SUMK_ERR_WORKSPACE; nothing is launched on any error.  Workspace: about 12 T (2 w + 64) bytes per video for the
 * band, plus 56 T D bytes of activations and gradients and 128 D^2 bytes of split-K slab for the VASNet pair. */
size_t sumk_attn_band_train_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture);
int sumk_attn_band_forward_train(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                 int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale, int32_t ignore_self,
                                 int32_t aperture, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* ctx, int32_t ldc,
                                 void* workspace, size_t workspace_bytes, void* stream);
int sumk_attn_band_backward(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, const float* dctx,
                            int32_t lddc, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                            int32_t ignore_self, int32_t aperture, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* dQ,
                            int32_t lddq, float* dK, int32_t lddk, float* dV, int32_t lddv, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t sumk_vasnet_band_train_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t aperture);
int sumk_vasnet_forward_band_train(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                   const sumk_vasnet_weights* w, const sumk_vasnet_opts* opts, float* scores, void* workspace,
                                   size_t workspace_bytes, void* stream);
struct sumk_vasnet_grads;
int sumk_vasnet_backward_band(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                              const sumk_vasnet_weights* w, const sumk_vasnet_opts* opts, const float* dscores,
                              const struct sumk_vasnet_grads* grads, float* dx, void* workspace, size_t workspace_bytes, void* stream,
                              void* tail_grads_ready_event);

/* Weight-plane block of sumk_vasnet_opts::wplanes: bytes (0 = D or n_planes not eligible: D % 256, n_planes 2 or 3), and the build --
 * planes of [Wq; Wk; Wv] (Wvo != NULL: [Wq; Wk; Wvo], the folded path of sumk_vasnet_forward_folded), of Wo, of k1's weight with the
 * LayerNorm gain folded in (W1 diag(ln_w)), and the three per-column vectors of the fused tail.  256-byte aligned device buffer; redo
 * after every weight change. */
size_t sumk_vasnet_wplanes_bytes(int32_t D, int32_t n_planes);
int sumk_vasnet_wplanes_build(int32_t D, const sumk_vasnet_weights* w, const float* Wvo, int32_t n_planes, void* out, size_t out_bytes,
                              void* stream);

/* Problem tables of a batch, separately (sumk_vasnet_opts::tables): size, and the one-time build (the setup kernels of a call, run into
 * `tables` instead of the workspace).  256-byte aligned device buffer. */
size_t sumk_vasnet_tables_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host);
int sumk_vasnet_build_tables(int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t training,
                             int32_t precision, void* tables, size_t tables_bytes, void* stream);

/* Replaces VASNet.forward (vasnet.py:92-148) for a packed batch: x (n_rows,D) -> scores (n_rows,), sigmoid
 * outputs in (0,1).  If pos_rows != NULL, x[r,:] += pos_table[pos_rows[r],:] is applied IN PLACE first
 * (vasnet.py:106-112 mutates the caller's tensor the same way).  When training != 0 the workspace keeps the
 * intermediates sumk_vasnet_backward consumes. */
int sumk_vasnet_forward(float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host,
                        const int32_t* seq_off_dev, const sumk_vasnet_weights* w,
                        const sumk_vasnet_opts* opts, const float* pos_table, const int32_t* pos_rows,
                        float* scores, void* workspace, size_t workspace_bytes, int32_t training,
                        void* stream);

/* Inference with the value and output projections folded: Wvo (D,D) = Wo . Wv, computed once per weight change by the caller
 * (sumk_gemm_nn(Wo, Wv, Wvo, D, D, D)).  (alpha V) Wo^T = alpha (X Wvo^T): the out-projection GEMM of vasnet.py:132 disappears
 * (18 % of the step's FLOPs); results equal sumk_vasnet_forward's up to fp32 re-association (~1e-6 on scores).  Opt-in
 * (VASNet(fold_vo=True)): the default path keeps the reference's operation order. */
int sumk_vasnet_forward_folded(float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host,
                               const int32_t* seq_off_dev, const sumk_vasnet_weights* w, const float* Wvo,
                               const sumk_vasnet_opts* opts, const float* pos_table, const int32_t* pos_rows,
                               float* scores, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ BiLSTM
 * One bidirectional LSTM layer (torch.nn.LSTM semantics: gates i,f,g,o; h0=c0=0), as used by DSN
 * (summarizer/models/dsn.py:23-27,45) and sLSTM (summarizer/models/sumgan.py:27-32,43).
 * dir 0 = forward, dir 1 = reverse.  Output h (n_rows, 2H) = [h_fwd || h_rev] per frame. */
typedef struct sumk_lstm_layer_weights {
  const float* w_ih[2]; /* (4H, In)  weight_ih_l{k}[_reverse] */
  const float* w_hh[2]; /* (4H, H)   weight_hh_l{k}[_reverse] */
  const float* b_ih[2]; /* (4H)      bias_ih_l{k}[_reverse]   */
  const float* b_hh[2]; /* (4H)      bias_hh_l{k}[_reverse]   */
  /* Optional, all three or none (zero-initialise the struct otherwise): inference in SUMK_PRECISION_BF16X6 / BF16X3 then runs the
     input projection of dsn.py:45 / sumgan.py:43 on the plane-aware wide GEMM (csrc/gemm_pw.hip) -- x_planes: the "KB planes" of x
     (n_rows x In, sumk_split_planes); w_planes: the block sumk_bilstm_wplanes_build wrote for THESE weights (planes of
     [w_ih[0]; w_ih[1]] and the summed biases).  Needs 8 H % 256 == 0, In % 32 == 0, In >= 128, n_rows >= 1024. */
  const void* x_planes;
  const void* w_planes;
} sumk_lstm_layer_weights;

/* Weight-plane block of sumk_lstm_layer_weights::w_planes: bytes (0 = not eligible) and the build (redo after a weight change). */
size_t sumk_bilstm_wplanes_bytes(int32_t In, int32_t H, int32_t n_planes);
int sumk_bilstm_wplanes_build(int32_t In, int32_t H, const sumk_lstm_layer_weights* w, int32_t n_planes, void* out, size_t out_bytes, void* stream);

size_t sumk_bilstm_workspace_bytes(int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host, int32_t training);
/* precision: SUMK_PRECISION_FP32, or SUMK_PRECISION_BF16X3 / SUMK_PRECISION_BF16X6 for the input projection (and, for 256 < H <= 1024, the
 * recurrent product: inference only for BF16X6) in the split-bf16 arithmetics described at sumk_vasnet_opts.  With w->x_planes / w->w_planes given
 * (inference) the projection runs on operand planes in front of the recurrence.  The workspace of 256 < H <= 1024 holds the
 * forward recurrence's exchange buffer (1 MB per 64 videos): ask sumk_bilstm_workspace_bytes again after upgrading the library. */
int sumk_bilstm_layer_forward(const float* x, int32_t In, int32_t H, int32_t n_seq,
                              const int32_t* seq_off_host, const int32_t* seq_off_dev,
                              const sumk_lstm_layer_weights* w, float* h_out,
                              void* workspace, size_t workspace_bytes, int32_t training, int32_t precision, void* stream);

/* Per-frame head shared by DSN (dsn.py:34-36,46: Linear(2H,1)+Sigmoid) and sLSTM (sumgan.py:33-34,44-45):
 * scores[r] = sigmoid(dot(h[r,:F], w) + b[0]). */
int sumk_frame_head_forward(const float* h, int32_t n_rows, int32_t F, const float* w, const float* b,
                            float* scores, void* stream);

/* Gradients of sum_r dscores[r]*scores[r] w.r.t. every weight (same struct, non-const targets) and,
 * optionally (dx != NULL), the input.  Must follow a training-mode forward on the same workspace.
 * Gradients are ACCUMULATED into grads (caller zeroes them), matching autograd's .grad semantics. */
typedef struct sumk_vasnet_grads {
  float* Wk; float* Wq; float* Wv; float* Wo; float* W1; float* b1; float* w2; float* b2; float* ln_w; float* ln_b;
} sumk_vasnet_grads;
int sumk_vasnet_backward(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host,
                         const int32_t* seq_off_dev, const sumk_vasnet_weights* w,
                         const sumk_vasnet_opts* opts, const float* dscores, const sumk_vasnet_grads* grads,
                         float* dx, void* workspace, size_t workspace_bytes, void* stream,
                         void* tail_grads_ready_event);
/* tail_grads_ready_event: NULL, or a hipEvent_t recorded on `stream` once the gradients of Wo, W1, b1, w2 and b2 are final
 * (before the attention backward and the Q/K/V weight gradients run): a data-parallel caller overlaps the all-reduce of
 * that part of its gradient bucket with the rest of this call (summarizer_amd/training.py: FlatAdam.reduce_tail_async). */

/* Synchronises `stream` and returns an error if a persistent recurrence kernel that used this workspace reported a
 * timed-out hand-off (outputs invalid).  Per-workspace word: valid until the next call reuses the workspace; the test-suite
 * (SUMK_CHECK=1) calls it after every recurrent layer.  Production code uses sumk_health_check below. */
int sumk_bilstm_check(const void* workspace, int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host,
                      int32_t training, int32_t after_backward, void* stream);
/* Sticky, workspace-free variant: synchronises `stream` and fails if ANY persistent recurrence kernel on the current device
 * timed out since the previous call (then resets the device-side word).  The Python trainers / scorers call it at the host
 * synchronisation points they already have (score D2H in Trainer.test / predict_dataset / StreamingScorer, per-epoch loss). */
int sumk_health_check(void* stream);

typedef struct sumk_lstm_layer_grads {
  float* w_ih[2]; float* w_hh[2]; float* b_ih[2]; float* b_hh[2];
  /* NULL (zero-initialise the struct), or a hipEvent_t the call RECORDS on `stream` once both bias gradients and the REVERSE direction's
     weight gradients (w_ih[1], w_hh[1]) are final -- before the forward direction's weight-gradient GEMMs run.  A data-parallel caller whose
     gradient bucket ends with [reverse direction | head] (the parameter order of DSN, dsn.py:23-36) can all-reduce that half on a side stream
     under the remaining GEMMs (training.FlatAdam.reduce_tail_async).  With the event set the two directions' dW_ih run as two launches
     (reverse first) instead of one. */
  void* tail_ready_event;
} sumk_lstm_layer_grads;
/* dh_out (n_rows,2H) -> accumulates weight grads; dx (n_rows,In) written if non-NULL.  Needs the workspace of
 * a training-mode sumk_bilstm_layer_forward and that call's h_out. */
int sumk_bilstm_layer_backward(const float* x, const float* h_out, const float* dh_out, int32_t In, int32_t H,
                               int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                               const sumk_lstm_layer_weights* w, const sumk_lstm_layer_grads* grads, float* dx,
                               void* workspace, size_t workspace_bytes, int32_t precision, void* stream);

/* ------------------------------------------------------------------------------------------------ GRU cell
 * The reference's optional `DSN(cell="gru")` (dsn.py:28-33, nn.GRU).  One fused element-wise step for B sequences, gate order
 * r, z, n (torch): gx = x_t W_ih^T + b_ih and gh = h_prev W_hh^T + b_hh are (B, 3H) (the host computes them with
 * sumk_linear_forward); mask (B) or NULL: 0 = the sequence has ended (h passes through, no gradient).  rzn (B, 3H) keeps the
 * gate values for sumk_gru_cell_backward, which returns d(gx), d(gh) and the DIRECT part of d(h_prev) (the caller adds dgh . W_hh).
 * This is the step path: it serves H > 256; smaller cells run the persistent layer below. */
int sumk_gru_cell_forward(const float* gx, const float* gh, const float* h_prev, const float* mask, float* h_out, float* rzn,
                          int32_t B, int32_t H, void* stream);
int sumk_gru_cell_backward(const float* dh, const float* rzn, const float* gh, const float* h_prev, const float* mask,
                           float* dgx, float* dgh, float* dh_prev, int32_t B, int32_t H, void* stream);

/* ------------------------------------------------------------------------------------------------ BiGRU
 * One bidirectional GRU layer (torch.nn.GRU semantics: gates r,z,n; h0 = 0) of `DSN(cell="gru")` on a packed batch, H <= 256, H % 4 == 0,
 * In % 4 == 0: the input projection as one GEMM per direction, then ONE cooperative launch for every time step of every video and both
 * directions (csrc/gru_persist.hip); the backward call is one cooperative launch for the BPTT plus the weight-gradient GEMMs.
 * Same conventions as the BiLSTM calls above: dir 0 = forward, dir 1 = reverse, h (n_rows, 2H) = [h_fwd || h_rev], borrowed pointers,
 * caller-owned workspace.  A hidden size outside the domain is SUMK_ERR_ARG and a short workspace SUMK_ERR_WORKSPACE: the call never
 * takes another route by itself -- the caller chooses (summarizer_amd.kernels.bigru_eligible).  training = 0 saves nothing. */
typedef struct sumk_gru_layer_weights {
  const float* w_ih[2]; /* (3H, In)  weight_ih_l{k}[_reverse] */
  const float* w_hh[2]; /* (3H, H)   weight_hh_l{k}[_reverse] */
  const float* b_ih[2]; /* (3H)      bias_ih_l{k}[_reverse]   */
  const float* b_hh[2]; /* (3H)      bias_hh_l{k}[_reverse]   */
} sumk_gru_layer_weights;
typedef struct sumk_gru_layer_grads {
  float* w_ih[2]; float* w_hh[2]; float* b_ih[2]; float* b_hh[2];
} sumk_gru_layer_grads;
size_t sumk_bigru_workspace_bytes(int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host, int32_t training);
/* precision: the arithmetic of the projection and gradient GEMMs (as sumk_bilstm_layer_forward); the recurrent products are exact fp32 MFMA. */
int sumk_bigru_layer_forward(const float* x, int32_t In, int32_t H, int32_t n_seq,
                             const int32_t* seq_off_host, const int32_t* seq_off_dev,
                             const sumk_gru_layer_weights* w, float* h_out,
                             void* workspace, size_t workspace_bytes, int32_t training, int32_t precision, void* stream);
/* dh_out (n_rows,2H) -> ACCUMULATES the weight gradients; dx (n_rows,In) written if non-NULL.  Needs the workspace of a training-mode
 * sumk_bigru_layer_forward and that call's h_out. */
int sumk_bigru_layer_backward(const float* x, const float* h_out, const float* dh_out, int32_t In, int32_t H,
                              int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                              const sumk_gru_layer_weights* w, const sumk_gru_layer_grads* grads, float* dx,
                              void* workspace, size_t workspace_bytes, int32_t precision, void* stream);
/* sumk_bilstm_check for a BiGRU workspace. */
int sumk_bigru_check(const void* workspace, int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host,
                     int32_t training, int32_t after_backward, void* stream);

/* ------------------------------------------------------------------------------------------------ unidirectional LSTM layer
 * One forward-running nn.LSTM(bidirectional=False) layer with an optional initial state and the final state as an output:
 * the layers of SumGAN's eLSTM / dLSTM / cLSTM (summarizer/models/sumgan.py:48-115,185-210).  Packed batch as above;
 * h0 / c0 / h_last / c_last / dh_last / dc_last / dh0 / dc0 are (n_seq, H) and may be NULL (zeros / not wanted). */
typedef struct sumk_lstm_dir_weights { const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; } sumk_lstm_dir_weights;
typedef struct sumk_lstm_dir_grads { float* w_ih; float* w_hh; float* b_ih; float* b_hh; } sumk_lstm_dir_grads;
size_t sumk_lstm_workspace_bytes(int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host, int32_t training);
int sumk_lstm_layer_forward(const float* x, int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host,
                            const int32_t* seq_off_dev, const sumk_lstm_dir_weights* w, const float* h0, const float* c0,
                            float* h_out, float* h_last, float* c_last, void* workspace, size_t workspace_bytes,
                            int32_t training, int32_t precision, void* stream);
/* Gradients ACCUMULATE into grads; dx (n_rows, In) written if non-NULL; dh_out may be NULL (no per-step upstream gradient).
 * Needs the workspace of a training-mode sumk_lstm_layer_forward, that call's h_out and the same c0. */
int sumk_lstm_layer_backward(const float* x, const float* h_out, const float* dh_out, const float* dh_last, const float* dc_last,
                             int32_t In, int32_t H, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                             const sumk_lstm_dir_weights* w, const float* c0, const sumk_lstm_dir_grads* grads, float* dx,
                             float* dh0, float* dc0, void* workspace, size_t workspace_bytes, int32_t precision, void* stream);

/* Step-wise decoder = SumGAN's dLSTM (sumgan.py:74-115): an n_layers-deep forward-running LSTM (input size == H) whose
 * input at step t is its own top-layer output of step t-1 (zeros at t = 0), started from (h0, c0) (n_layers, n_seq, H) or
 * NULL.  out (n_rows, H) = top-layer outputs in time order (the module flips them, sumgan.py:114).  w / grads: n_layers
 * entries.  backward: needs the forward's workspace and out; grads ACCUMULATE; dh0 / dc0 (n_layers, n_seq, H) or NULL. */
size_t sumk_lstm_decoder_workspace_bytes(int32_t H, int32_t n_layers, int32_t n_seq, const int32_t* seq_off_host);
int sumk_lstm_decoder_forward(int32_t H, int32_t n_layers, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                              const sumk_lstm_dir_weights* w, const float* h0, const float* c0, float* out, void* workspace,
                              size_t workspace_bytes, void* stream);
int sumk_lstm_decoder_backward(int32_t H, int32_t n_layers, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                               const sumk_lstm_dir_weights* w, const float* c0, const float* out, const float* dout,
                               const sumk_lstm_dir_grads* grads, float* dh0, float* dc0, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Dense layer y (M,N) = x (M,K) w^T + b for the small Linear layers around the LSTM stacks (sumgan.py:58-59,84); w is (N,K)
 * as in nn.Linear, b may be NULL.  backward: dx (M,K) written if non-NULL, dw (N,K) / db (N) ACCUMULATED if non-NULL. */
size_t sumk_linear_workspace_bytes(int32_t N, int32_t K);
int sumk_linear_forward(const float* x, const float* w, const float* b, float* y, int32_t M, int32_t N, int32_t K,
                        void* workspace, size_t workspace_bytes, int32_t precision, void* stream);
int sumk_linear_backward(const float* x, const float* w, const float* dy, int32_t M, int32_t N, int32_t K, float* dx, float* dw,
                         float* db, void* workspace, size_t workspace_bytes, int32_t precision, void* stream);

/* dh[r,:] = ds[r]*s(1-s)*w ; dw += sum_r ds*s(1-s)*h[r,:] ; db += sum_r ds*s(1-s) */
size_t sumk_frame_head_workspace_bytes(int32_t F);
int sumk_frame_head_backward(const float* h, const float* scores, const float* dscores, int32_t n_rows,
                             int32_t F, const float* w, float* dh, float* dw, float* db, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ Transformer scorer
 * The reference's Transformer-encoder scorer (summarizer/models/transformer.py:74-103): n_layers stock
 * nn.TransformerEncoderLayer (post-norm, ReLU, dim_feedforward F), final norm = the SHARED layer_norm (also applied after
 * k1), optional extra residual (more_residuals), k1 + ReLU + LN + k2 + sigmoid.  Weights as torch stores them. */
typedef struct sumk_tf_layer_weights {
  const float* in_proj_w;  const float* in_proj_b;    /* (3D,D),(3D)  self_attn.in_proj_{weight,bias} */
  const float* out_proj_w; const float* out_proj_b;   /* (D,D),(D)    self_attn.out_proj              */
  const float* lin1_w; const float* lin1_b;           /* (F,D),(F)    linear1                          */
  const float* lin2_w; const float* lin2_b;           /* (D,F),(D)    linear2                          */
  const float* norm1_w; const float* norm1_b; const float* norm2_w; const float* norm2_b;   /* (D) */
} sumk_tf_layer_weights;
typedef struct sumk_tf_head_weights {
  const float* ln_w; const float* ln_b;               /* (D) layer_norm (== transformer_encoder.norm)  transformer.py:47,50,100 */
  const float* k1_w; const float* k1_b;               /* (D,D),(D)                                     transformer.py:52 */
  const float* k2_w; const float* k2_b;               /* (D),(1)                                       transformer.py:53 */
} sumk_tf_head_weights;
typedef struct sumk_tf_opts {
  float layer_eps;        /* LayerNorm eps inside the encoder layers (torch default 1e-5)                       */
  float final_eps;        /* eps of the shared layer_norm (constructor argument `epsilon`)    transformer.py:47  */
  int32_t more_residuals; /* encoder_out += x                                                  transformer.py:94  */
  float layer_dropout_p;  /* training: dropout inside the encoder layers (0.1)                 transformer.py:49  */
  float head_dropout_p;   /* training: dropout after relu(k1) (0.5)                            transformer.py:46,99 */
  uint64_t seed;          /* keep-masks are a pure function of (seed, site, element), as for VASNet               */
  int32_t precision;      /* SUMK_PRECISION_*, as in sumk_vasnet_opts                                             */
  const void* wplanes;    /* inference in BF16X6 / BF16X3: the weights as bf16 planes (sumk_transformer_wplanes_build, 256-byte
                             aligned) -> every projection of the stack runs on the plane GEMM; NULL: the in-loop split kernels */
} sumk_tf_opts;
size_t sumk_transformer_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                        const int32_t* seq_off_host, int32_t training);
/* the same plus the two activation-plane buffers of the plane path (inference, BF16X6 / BF16X3, D and F multiples of 256,
 * at least 128 frames); equal to sumk_transformer_workspace_bytes otherwise */
size_t sumk_transformer_workspace_bytes_for(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                            const int32_t* seq_off_host, int32_t training, int32_t precision);
/* Weight planes of the encoder stack and k1 (transformer.py:49-53: in_proj, out_proj, linear1, linear2 of every layer; k1) for
 * n_planes = 3 (BF16X6) or 2 (BF16X3); 0 bytes = not eligible.  Rebuild after every weight change. */
size_t sumk_transformer_wplanes_bytes(int32_t D, int32_t F, int32_t n_layers, int32_t n_planes);
int sumk_transformer_wplanes_build(int32_t D, int32_t F, int32_t n_layers, const sumk_tf_layer_weights* layers,
                                   const sumk_tf_head_weights* head, int32_t n_planes, void* out, size_t out_bytes,
                                   void* stream);
/* x (n_rows,D) packed -> scores (n_rows,).  pos_table/pos_rows as in sumk_vasnet_forward (in-place add, transformer.py:83-89).
 * training != 0 keeps every layer's activations in the workspace for sumk_transformer_backward. */
int sumk_transformer_forward(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                             const int32_t* seq_off_host, const int32_t* seq_off_dev,
                             const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                             const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows, float* scores,
                             void* workspace, size_t workspace_bytes, int32_t training, void* stream);
/* Multi-head attention WITHOUT the (T x T) logits (csrc/attn_stream.hip), exact fp32, no mask, for a packed batch: per video v and head h
 *   ctx[rows of v, h dh : (h + 1) dh] = softmax_j(scale Q_h K_h^T) V_h,   dh = D / n_heads,
 * with head h at column h * dh of Q, K, V and ctx (leading dimensions >= D and % 4 == 0, pointers 16-byte aligned: the in-place
 * [Q | K | V] buffer with ld = 3 D works) and one segment table for Q and K / V.  lse: NULL, or (n_rows, n_heads) floats that receive
 * log sum_j exp(scale q . k_j) per (row, head).  One setup launch and one attention launch -- a workgroup per (128-row query strip,
 * head) walks the video's 64-key tiles in ascending order with an online softmax rescaled every tile; logits live in MFMA accumulator
 * registers only, so nothing of size T x T exists and the workspace is 16 bytes per video.  No cooperative launch, no atomics: every
 * call gives the same bits, and the call only enqueues work (it may be captured into a HIP graph).  Every global offset is 64-bit.
 * Limits: dh % 4 == 0 and dh <= 256; 1 <= T < 2^20 frames per video; at most 65 535 videos; scale positive and finite.  Anything else
 * returns SUMK_ERR_ARG, a short workspace SUMK_ERR_WORKSPACE; both set sumk_last_error() and launch nothing.  NaN in a Q row gives NaN
 * in that row of ctx; NaN in a K or V row reaches the rows of its own video (and the heads whose columns hold it) only.
 * The size queries are host arithmetic (0 = bad arguments).
 * sumk_transformer_forward_stream: the inference of sumk_transformer_forward (same arguments without `training`) with the attention
 * of every layer on that launch and no logits block in its workspace (sumk_transformer_stream_workspace_bytes: O(n_rows (D + F))).
 * opts->precision must be SUMK_PRECISION_FP32, opts->wplanes NULL and both dropout probabilities 0; the limits above apply. */
size_t sumk_attn_stream_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host);
int sumk_attn_stream(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                     int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                     float* ctx, int32_t ldc, float* lse, void* workspace, size_t workspace_bytes, void* stream);
size_t sumk_transformer_stream_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                               const int32_t* seq_off_host);
int sumk_transformer_forward_stream(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                    const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                    const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                    const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows, float* scores,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* sumk_attn_stream in the bf16x3 arithmetic (csrc/attn_stream_split.hip), scoring only: Q, K and V are split once per call into two
 * bf16 planes (hi = bf16(x) to nearest even, lo = bf16(x - hi)) in the workspace -- 4 bytes per staged element, videos padded to whole
 * 64-key tiles, head widths to 32 / 64 / 128 columns -- and both products run as hi.hi + hi.lo + lo.hi on the bf16 MFMA with fp32
 * accumulation; the softmax is sumk_attn_stream's in fp32, the weights are split in registers.  Three launches (descriptors, split,
 * attention), no cooperative launch, no atomics: same bits every call, capturable.  `precision` / `attention_precision` accept
 * SUMK_PRECISION_BF16X3 only (any other value: SUMK_ERR_ARG with the value in the message).  Limits: dh % 8 == 0 and dh <= 128, the
 * workspace 16-byte aligned, otherwise sumk_attn_stream's; errors as there.  The NaN rules are sumk_attn_stream's.
 * sumk_transformer_forward_stream_split: sumk_transformer_forward_stream with every layer's attention on that call; the projections stay
 * exact fp32 (opts->precision must be SUMK_PRECISION_FP32).  Workspace: the stream carve + the planes of one layer's [Q | K | V]. */
size_t sumk_attn_stream_split_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, int32_t precision);
int sumk_attn_stream_split(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                           int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                           int32_t precision, float* ctx, int32_t ldc, float* lse, void* workspace, size_t workspace_bytes, void* stream);
size_t sumk_transformer_stream_split_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                     const int32_t* seq_off_host, int32_t attention_precision);
int sumk_transformer_forward_stream_split(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                          const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                          const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                          const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows, float* scores,
                                          int32_t attention_precision, void* workspace, size_t workspace_bytes, void* stream);
/* Gradient targets, same shapes as the weights; ACCUMULATED into (caller zeroes them). */
typedef struct sumk_tf_layer_grads {
  float* in_proj_w; float* in_proj_b; float* out_proj_w; float* out_proj_b; float* lin1_w; float* lin1_b;
  float* lin2_w; float* lin2_b; float* norm1_w; float* norm1_b; float* norm2_w; float* norm2_b;
} sumk_tf_layer_grads;
typedef struct sumk_tf_head_grads { float* ln_w; float* ln_b; float* k1_w; float* k1_b; float* k2_w; float* k2_b; } sumk_tf_head_grads;
/* Backward of sum_r dscores[r]*scores[r] (loss.backward(), transformer.py:163); must follow a training-mode forward on the
 * same workspace.  dx (n_rows,D) is written if non-NULL. */
int sumk_transformer_backward(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                              const int32_t* seq_off_host, const int32_t* seq_off_dev,
                              const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                              const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* layer_grads,
                              const sumk_tf_head_grads* head_grads, float* dx, void* workspace, size_t workspace_bytes,
                              void* stream);
/* Training on the stream form: sumk_attn_stream under autograd, still without anything of size T x T.
 * sumk_attn_stream_train: sumk_attn_stream with dropout of the weights (a~ = keep ? alpha / (1 - p) : 0, keep = the library's hash of
 * (seed, site, ((packed row * n_heads + h) << 20) | key), the index the dense path uses, so one seed gives both paths the same masks)
 * and stats (n_rows, n_heads, 2) floats, 8-byte aligned: the row maximum m of the scaled logits and l = sum_j exp(s_j - m) per (row,
 * head).  With dropout_p == 0 ctx has the bits of sumk_attn_stream.  Workspace: sumk_attn_stream_workspace_bytes.
 * sumk_attn_stream_backward: dQ, dK, dV (written, not accumulated; they may be the three column blocks of one (n_rows, 3 D) buffer) from
 * Q, K, V, the forward's ctx and stats, and dctx, with the forward's scale, dropout_p, seed and site.  Three launches after the setup:
 * delta = dctx . ctx per (row, head); a pass per (128-row query strip, head) over the video's 64-key tiles for dQ; a pass per (128-row
 * key strip, head) over its 64-query tiles for dK and dV.  The weights are recomputed per tile from Q, K and stats and the masks
 * regenerated in registers; no atomics, every call gives the same bits; seven products of 2 T^2 D FLOP instead of five.  Workspace
 * (sumk_attn_stream_backward_workspace_bytes): the descriptors + 4 bytes per (row, head).
 * Limits as sumk_attn_stream, but dh <= 128 in the backward (and hence in the transformer entries below) and dropout_p in [0, 1).
 * sumk_transformer_forward_stream_train / sumk_transformer_backward_stream: the training forward and the backward of
 * sumk_transformer_forward / sumk_transformer_backward (same arguments, dropout sites and gradient accumulation) with every layer's
 * attention on these launches; the workspace (sumk_transformer_stream_train_workspace_bytes) is the dense training carve without the
 * logits scratch and the two heads x T x T blocks per layer, plus stats per layer.  Exact fp32 only, opts->wplanes NULL. */
int sumk_attn_stream_train(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                           int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                           float dropout_p, uint64_t seed, uint32_t site, float* ctx, int32_t ldc, float* stats, void* workspace,
                           size_t workspace_bytes, void* stream);
size_t sumk_attn_stream_backward_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host);
int sumk_attn_stream_backward(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, const float* ctx,
                              int32_t ldc, const float* dctx, int32_t ldd, const float* stats, int32_t D, int32_t n_heads,
                              int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale, float dropout_p,
                              uint64_t seed, uint32_t site, float* dQ, int32_t lddq, float* dK, int32_t lddk, float* dV, int32_t lddv,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The two calls above in the bf16x3 arithmetic of sumk_attn_stream_split (csrc/attn_stream_split.hip: training forward;
 * csrc/attn_stream_split_bwd.hip: backward), opt-in.  Every operand is two bf16 planes, every one of the seven products hi.hi + hi.lo +
 * lo.hi with fp32 accumulation on the bf16 MFMA; softmax, masks and the dS arithmetic stay in fp32, and a~ and dS are split in registers.
 * sumk_attn_stream_split_train: sumk_attn_stream_train's arguments + `precision`; masks, mask index and stats as there; with
 * dropout_p == 0 ctx has the bits of sumk_attn_stream_split.  Workspace: sumk_attn_stream_split_workspace_bytes.
 * sumk_attn_stream_split_backward: sumk_attn_stream_backward's arguments + `precision`.  delta is the fp32 launch; one pass splits Q, K,
 * V and dctx into planes (row-major for all four, transposed per 64-row tile for Q, K and dctx: 28 bytes per (padded row, staged column));
 * the dQ and dK / dV passes have the structure of the fp32 backward and are deterministic.  Workspace
 * (sumk_attn_stream_split_backward_workspace_bytes): descriptors + delta + those planes, 16-byte aligned.
 * `precision` accepts SUMK_PRECISION_BF16X3 only (any other value: SUMK_ERR_ARG with the value in the message).  Limits: dh % 8 == 0 and
 * dh <= 128 (refused with the head width in the message), otherwise those of the fp32 calls. */
int sumk_attn_stream_split_train(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, int32_t D,
                                 int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                                 float dropout_p, uint64_t seed, uint32_t site, float* ctx, int32_t ldc, float* stats, void* workspace,
                                 size_t workspace_bytes, void* stream, int32_t precision);
size_t sumk_attn_stream_split_backward_workspace_bytes(int32_t D, int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host,
                                                       int32_t precision);
int sumk_attn_stream_split_backward(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv,
                                    const float* ctx, int32_t ldc, const float* dctx, int32_t ldd, const float* stats, int32_t D,
                                    int32_t n_heads, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, float scale,
                                    float dropout_p, uint64_t seed, uint32_t site, float* dQ, int32_t lddq, float* dK, int32_t lddk,
                                    float* dV, int32_t lddv, void* workspace, size_t workspace_bytes, void* stream, int32_t precision);
/* sumk_transformer_forward_stream_split_train / sumk_transformer_backward_stream_split: the stream training entries below with every
 * layer's attention on the two calls above (`attention_precision`: SUMK_PRECISION_BF16X3 only); projections and everything else stay
 * exact fp32 (opts->precision must be SUMK_PRECISION_FP32, opts->wplanes NULL); same dropout sites and masks.  Workspace
 * (sumk_transformer_stream_split_train_workspace_bytes): the stream training carve + sumk_attn_stream_split_backward_workspace_bytes --
 * the planes are those of one layer, re-split in the backward from the saved [Q | K | V]; the state kept per layer is unchanged. */
size_t sumk_transformer_stream_split_train_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                           const int32_t* seq_off_host, int32_t attention_precision);
int sumk_transformer_forward_stream_split_train(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                                const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                                const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows, float* scores,
                                                int32_t attention_precision, void* workspace, size_t workspace_bytes, void* stream);
int sumk_transformer_backward_stream_split(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                           const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                           const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                           const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* layer_grads,
                                           const sumk_tf_head_grads* head_grads, float* dx, int32_t attention_precision, void* workspace,
                                           size_t workspace_bytes, void* stream);
size_t sumk_transformer_stream_train_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                                     const int32_t* seq_off_host);
int sumk_transformer_forward_stream_train(float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                          const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                          const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                          const sumk_tf_opts* opts, const float* pos_table, const int32_t* pos_rows, float* scores,
                                          void* workspace, size_t workspace_bytes, void* stream);
int sumk_transformer_backward_stream(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                     const int32_t* seq_off_host, const int32_t* seq_off_dev,
                                     const sumk_tf_layer_weights* layers, const sumk_tf_head_weights* head,
                                     const sumk_tf_opts* opts, const float* dscores, const sumk_tf_layer_grads* layer_grads,
                                     const sumk_tf_head_grads* head_grads, float* dx, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* ------------------------------------------------------------------------------------------------ DSN reward
 * DSNTrainer.compute_reward (dsn.py:185-236) for E episodes of one or more packed videos:
 * actions (E, n_rows) of 0/1 floats -> reward (E, n_seq).  Zero picks -> 0 (dsn.py:199-203); one pick ->
 * r_div = 0 (dsn.py:211-214) and r_rep from that pick (the reference itself raises IndexError there). */
size_t sumk_dsn_reward_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t n_episodes);
int sumk_dsn_reward(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host,
                    const int32_t* seq_off_dev, const float* actions, int32_t n_episodes, int32_t far_sim,
                    int32_t temp_dist_thre, float* reward, void* workspace, size_t workspace_bytes, void* stream);
/* The same reward without the (T x T) Gram matrix (csrc/reward_stream.hip): every Gram tile is consumed in registers as the MFMA
 * produces it, so the workspace is O(n_episodes x n_rows) and a video may have up to 1 048 576 frames (n_rows < 2^31, D % 4 == 0,
 * x 16-byte aligned, any number of episodes; every offset into x is 64-bit).  Arguments, semantics, status codes and
 * sumk_last_error() as sumk_dsn_reward: a frame is picked where its action is non-zero (-0.0 is not a pick), no pick gives exactly
 * 0, one pick gives r_div = 0 with r_rep evaluated, a picked zero-norm frame among two or more picks gives NaN for that (episode,
 * video) only.  col_split: 0 = the library's plan (sumk_dsn_reward_stream_plan), 1..8 = that many splits of a video's 64-column
 * key tiles among workgroups (a video never gets more splits than it has key tiles); every split count gives a result within
 * rounding of the others, and one split count gives the same bits on every call.  The workspace size does not depend on col_split.
 * Episodes are served in chunks of SUMK_REWARD_STREAM_EC per pass over the tiles.  No cooperative launch, no float atomics;
 * the whole call may be captured into a HIP graph. */
#define SUMK_REWARD_STREAM_EC 8
size_t sumk_dsn_reward_stream_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t n_episodes);
int32_t sumk_dsn_reward_stream_plan(int32_t n_seq, const int32_t* seq_off_host);   /* the split count col_split = 0 stands for; 0 on a bad argument */
int sumk_dsn_reward_stream(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host,
                           const int32_t* seq_off_dev, const float* actions, int32_t n_episodes, int32_t far_sim,
                           int32_t temp_dist_thre, int32_t col_split, float* reward, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The loss glue of DSNTrainer.train for a packed batch (dsn.py:113-140), per video v:
 *   loss_per_video[v] = [ beta (mean_t p_t - eps_target)^2 - sum_e (rewards[e,v] - base[v]) mean_t log P(actions[e,t] | p_t) ] / E
 * with torch.distributions.Bernoulli's log_prob (probabilities clamped to [eps, 1 - eps], eps = float32 epsilon), and its
 * gradient w.r.t. the probabilities given dloss_per_video.  actions (E, n_rows), rewards (E, n_seq), base (n_seq); mean_probs
 * (n_seq) is written by the forward and read by the backward.  E <= 16.  The supervised BCE term of `sup=True` stays outside. */
int sumk_dsn_policy_loss_forward(const float* probs, const float* actions, const float* rewards, const float* base,
                                 int32_t n_seq, int32_t n_rows, const int32_t* seq_off_dev, int32_t n_episodes,
                                 float beta, float eps_target, float* loss_per_video, float* mean_probs, void* stream);
int sumk_dsn_policy_loss_backward(const float* probs, const float* actions, const float* rewards, const float* base,
                                  const float* mean_probs, const float* dloss_per_video, int32_t n_seq, int32_t n_rows,
                                  const int32_t* seq_off_dev, int32_t n_episodes, float beta, float eps_target,
                                  float* dprobs, void* stream);
/* nn.MSELoss per video of a packed batch (vasnet.py:209, transformer.py:161): mse_per_video[v] = mean_t (scores_t - target_t)^2,
 * and dscores_t = 2 (scores_t - target_t) / T_v * dmse_per_video[v]. */
int sumk_segment_mse_forward(const float* scores, const float* target, int32_t n_seq, const int32_t* seq_off_dev,
                             float* mse_per_video, void* stream);
int sumk_segment_mse_backward(const float* scores, const float* target, const float* dmse_per_video, int32_t n_seq,
                              const int32_t* seq_off_dev, float* dscores, void* stream);
/* The trainers' step loss in one launch each way (vasnet.py:209-212: mean over the videos of a step of nn.MSELoss per video):
 * loss[0] = scale * sum_v mse_per_video[v] (scale = 1 / videos of the step; the per-video values are written too and added in video order),
 * dscores_t = 2 (scores_t - target_t) / T_v * scale * dloss[0] (dloss: the device scalar autograd hands the backward).
 * `ticket`: one device word the caller zeroes ONCE and keeps for this batch; every launch leaves it zero (a block per video, the last
 * arriver adds); one launch at a time per word. */
int sumk_segment_mse_mean_forward(const float* scores, const float* target, int32_t n_seq, const int32_t* seq_off_dev, float scale,
                                  float* mse_per_video, float* loss, uint32_t* ticket, void* stream);
int sumk_segment_mse_mean_backward(const float* scores, const float* target, const float* dloss, float scale, int32_t n_seq,
                                   const int32_t* seq_off_dev, float* dscores, void* stream);

/* ------------------------------------------------------------------------------------------------ optimiser
 * torch.optim.Adam(lr, betas, eps, weight_decay) exactly as the trainers construct it (vasnet.py:181,
 * dsn.py:70-73): L2 weight decay folded into the gradient, bias-corrected moments.  One flat launch over
 * n elements; `step` is the 1-based step count.  grad_scale multiplies the gradient first (used for
 * clip_grad_norm_, dsn.py:145, and for the 1/world_size of a data-parallel average).  The betas are doubles: torch takes 1 - beta in
 * double before it rounds to fp32, and 1 - (float)0.999 is 1.3e-5 relative away from (float)0.001. */
int sumk_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, double beta1, double beta2, float eps, float weight_decay, int32_t step,
                   float grad_scale, void* stream);
/* The same step with NOTHING on the host: `state` is a 16-byte device block the caller zeroes once -- state[0] (int32) counts
 * the optimiser steps and is incremented by the call, state[1..3] are scratch -- so the bias correction follows a counter that
 * lives on the device, and when `sumsq` (device scalar from sumk_sumsq: the squared L2 norm of the UNscaled gradient) is
 * given, torch.nn.utils.clip_grad_norm_(params, max_norm) (dsn.py:145) is folded in without reading the norm back.  No host
 * synchronisation, captures into a HIP graph and replays with the right step count.  Same arithmetic as sumk_adam_step. */
int sumk_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, double beta1, double beta2, float eps, float weight_decay, int32_t* state,
                       float grad_scale, const float* sumsq, float max_norm, void* stream);
/* The same, and `grad` is left ZERO: the next step's optimizer.zero_grad() (vasnet.py:210, dsn.py:143) folded into the pass that reads
 * the gradient last -- one 21 MB fill launch less per step of a captured (HIP graph) training step. */
int sumk_adam_step_dev_zero_grad(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                 float lr, double beta1, double beta2, float eps, float weight_decay, int32_t* state,
                                 float grad_scale, const float* sumsq, float max_norm, void* stream);
/* out[0] += sum of squares of a flat buffer (for clip_grad_norm_), deterministic two-stage reduction.
 * workspace: sumk_sumsq_workspace_bytes() bytes of device scratch. */
size_t sumk_sumsq_workspace_bytes(void);
int sumk_sumsq(const float* v, int64_t n, float* out, void* workspace, void* stream);
/* Flat fp32 <-> bf16 casts (round to nearest even): in the mixed-precision training mode (SUMK_PRECISION_BF16) the gradient
 * bucket crosses the data-parallel all-reduce as bf16 -- 10.5 MB instead of 21 MB for VASNet -- and comes back into the fp32
 * bucket the optimiser reads.  No reference counterpart (the reference has no distributed code). */
int sumk_cast_f32_bf16(const float* src, void* dst_bf16, int64_t n, void* stream);
int sumk_cast_bf16_f32(const void* src_bf16, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------ logistic-regression step
 * One optimiser step of the logistic baseline (logistic.py:67-88) in ONE launch (csrc/logistic.hip): for the packed rows x (n_rows, D),
 * D % 4 == 0 and D <= 2048, and the min-max normalised target (n_rows,):
 *   s_r = sigmoid(x_r . w + b),  mse_per_video[v] = mean_t (s - t)^2,  loss[0] = scale * sum_v mse_per_video[v]  (scale = 1 / videos of
 *   the step: the step loss of sumk_segment_mse_mean_forward),  dW = sum_r g_r x_r,  db = sum_r g_r,
 *   g_r = 2 (s_r - t_r) / T_v * scale * s_r (1 - s_r).
 * The parameters are a flat bucket [w (D) | b | 3 floats of padding] (FlatAdam's layout for nn.Linear(D, 1)); flat_grad, exp_avg and
 * exp_avg_sq have the same D + 4 floats, all 16-byte aligned.  apply_adam != 0: torch.optim.Adam(lr, betas, eps, weight_decay) applied
 * to [w | b] with the arithmetic of sumk_adam_step_dev (state: its 16-byte device block; state[0] incremented), flat_grad not used.
 * apply_adam == 0: [dW | db] is ADDED to flat_grad (.grad semantics) and nothing else changes -- the data-parallel form (all-reduce,
 * then sumk_adam_step_dev).  scores: NULL or (n_rows,) for s.  Bit-deterministic (partials added in block order).  The call zeroes the
 * first 16 bytes of the workspace with hipMemsetAsync before the launch (one launch at a time per workspace). */
size_t sumk_logistic_step_workspace_bytes(int32_t n_rows, int32_t D);
int sumk_logistic_step(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                       const float* target, float* flat_param, float* flat_grad, float* exp_avg, float* exp_avg_sq, int32_t* state,
                       float lr, double beta1, double beta2, float eps, float weight_decay, float scale, int32_t apply_adam,
                       float* loss, float* mse_per_video, float* scores, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ generic
 * fp32 MFMA GEMM (the dominant kernel), exposed for tests and for bench.py's roofline probe:
 * C(M,N) = A(M,K) * B^T  with B given as (N,K) row-major ("NT", both operands K-contiguous). */
int sumk_gemm_nt(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, void* stream);
/* any of the three products (layout 0 = NT, 1 = NN, 2 = TN, operands as above) in the selected arithmetic
 * (SUMK_PRECISION_FP32 | SUMK_PRECISION_BF16X3) */
int sumk_gemm_prec(int32_t layout, const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int32_t precision,
                   void* stream);
/* The same three products with bf16 OPERANDS in device memory (fp32 accumulate and output): the GEMM of the mixed-precision
 * training step (csrc/gemm_b16.hip), exposed for tests and probes.  K-contiguous operands need K % 64 == 0, the others rows of
 * whole 16-byte chunks.  workspace == NULL: C = product.  workspace given (layout 2 only, 256-byte aligned, >= 8192 + 4 M N
 * bytes): deterministic split-K over a long K and C += product -- the weight-gradient form of vasnet.py:193-212's backward. */
int sumk_gemm_bf16src(int32_t layout, const void* A_bf16, const void* B_bf16, float* C, int32_t M, int32_t N, int32_t K,
                      void* workspace, size_t workspace_bytes, void* stream);
/* ---- Positional embeddings on packed batches (csrc/posembed.hip; vasnet.py:106-112, transformer.py:82-88 with one video per call).
 * sumk_pos_add_packed: y[off[v] + t, :] = x[off[v] + t, :] + table[t, :] for every video v of the batch, OUT OF PLACE (x is never
 * written; the position comes from the sequence offsets, there is no row-index array).  Up to three outputs, NULL = not wanted:
 *   out_f32   (n_rows, D) fp32 -- bit-equal to a plain fp32 add;
 *   out_bf16  (n_rows, D) bf16 -- the rounding of sumk_cast_f32_bf16 applied to that sum (sumk_vasnet_opts::x16);
 *   out_planes  the "KB planes" (below) of the (n_rows x D) sum with n_planes = 2 or 3, byte-equal to sumk_split_planes of it: every
 *             row up to the pitch is written (zeros behind n_rows); the caller clears the last 8192 bytes of the array as for
 *             sumk_split_planes.  The planes are made from x and the table in registers, not from an fp32 sum in memory.
 * D % 4 == 0 (planes: D % 16 == 0); 16-byte aligned buffers.  A video longer than table_rows, or any other bad argument, returns
 * SUMK_ERR_ARG and launches nothing.
 * sumk_pos_table_grad: dtable[t, :] += sum over the videos with more than t frames of dx[off[v] + t, :] -- the gradient of a learnable
 * table (nn.Embedding, vasnet.py:42).  One thread owns each (t, 4 columns): it starts from the value dtable holds and adds the videos
 * in ascending order with plain fp32 adds (no atomics: bit-deterministic).  Rows at or above the longest video are not touched. */
int sumk_pos_add_packed(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                        const float* table, int32_t table_rows, float* out_f32, void* out_bf16, void* out_planes,
                        int32_t n_planes, void* stream);
int sumk_pos_table_grad(const float* dx, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                        float* dtable, int32_t table_rows, void* stream);
/* ---- "KB planes": the operand format of the plane-aware wide GEMM behind SUMK_PRECISION_BF16X6 / BF16X3 scoring (csrc/gemm_pw.hip).
 * An fp32 matrix (rows x K, K % 16 == 0) as n_planes = 3 (x = x1 + x2 + x3 exactly) or 2 (hi + lo) bf16 planes, k-blocked:
 *   byte offset of (row, k, plane p) = (((k / 16) * n_planes + p) * 2 + (k / 8) % 2) * 16 * pitch + row * 16 + (k % 8) * 2,
 *   pitch = rows rounded up to 64.   Written once per dataset (x), per weight change (weights) or by the producing kernel's epilogue;
 * no reference counterpart (the reference multiplies fp32 tensors with torch.matmul, vasnet.py:114-131).
 * sumk_planes_bytes: device bytes of one plane array (0 = bad arguments).  sumk_split_planes: fp32 (rows x K, leading dimension ld)
 * -> planes.  sumk_gemm_planes (tests / bench probe): C(M,N) fp32 = A . B^T from two plane arrays built for a_rows / b_rows rows
 * (N % 256 == 0, K % 32 == 0, K >= 128).  variant: 1 = every wave of the 32x32x16 kernel refills its stage right behind the barrier,
 * 10 = waves 0-3 do, any other value = the product's schedule; 32 also keeps two planes on the 32x32x16 kernel (the product runs them on
 * the 16x16x32 kernel when K >= 160). */
size_t sumk_planes_bytes(int64_t rows, int32_t K, int32_t n_planes);
int sumk_split_planes(const float* src, int64_t rows, int32_t K, int32_t ld, int32_t n_planes, void* planes, void* stream);
int sumk_gemm_planes(const void* A_planes, int64_t a_rows, const void* B_planes, int64_t b_rows, float* C, int32_t M, int32_t N, int32_t K,
                     int32_t n_planes, int32_t variant, void* stream);
/* Per-video attention on planes (csrc/attn_pw.hip; tests / probes -- sumk_vasnet_forward runs the same two launches): from the KB planes
 * of the (rows x 3 D) matrix [Q | K | V], per video s (frames seq_off[s] .. seq_off[s + 1], at most 320):
 *   alpha = softmax(mask(Q K^T * scale)) (vasnet.py:118-129) -> alpha_planes (rows = frames, k = key index inside the video, row pitch of
 *   the input planes; sumk_attn_planes_alpha_bytes) and, when E != NULL, fp32 alpha as (T x roundup4(T)) blocks back to back;
 *   ctx_planes != NULL: context = alpha V (vasnet.py:131) as KB planes of the (rows x D) matrix.  Synchronises the stream (test entry). */
size_t sumk_attn_planes_alpha_bytes(int64_t rows, int32_t t_max, int32_t n_planes);
int sumk_attn_planes(const void* qkv_planes, int64_t rows, int32_t D, int32_t n_planes, int32_t n_seq, const int32_t* seq_off_host,
                     float scale, int32_t ignore_self, int32_t aperture, float* E, void* alpha_planes, void* ctx_planes, void* stream);
/* Fused attention strips of the bf16-source training step (csrc/attn_b16.hip) on their own: FOR TESTS AND PROBES ONLY -- the product
 * reaches the same launch through sumk_vasnet_forward / sumk_vasnet_backward with precision bf16, this entry allocates, synchronises
 * the stream and frees on every call.  All 16-bit arrays are bf16; per video s of T = seq_off[s + 1] - seq_off[s] <= 320 frames
 * (D a multiple of 256, every ld >= D and a multiple of 8, every pointer 16-byte aligned):
 *   backward == 0: A = Q, B = K, C = V (rows x D inside rows of ld elements).  E (written) = alpha = softmax(mask(Q K^T * scale)), fp32
 *     (T x roundup4(T)) blocks back to back, pad columns 0; P16 (written) = bf16(dropout(alpha)), (T x roundup64(T)) blocks back to
 *     back, pad columns 0; O16 (written, rows x D inside rows of ldo) = bf16(P16 V).  vasnet.py:118-131.
 *   backward != 0: A = dCTX, B = V, C = K; E (read) = alpha of the forward; P16 (written) = bf16(dS),
 *     dS = scale * alpha * (dropout'(dCTX V^T) - sum_j dropout'(dCTX V^T)_j alpha_j); O16 (written) = bf16(P16 K) = dQ.
 * Dropout keeps element (packed row r, key j) when dropout_keep(seed, site 0, (r << 20) | j) says so, scaled by 1 / (1 - dropout_p).
 * sumk_attn_strips_b16_sizes: the element counts of E and P16 for a batch (host arithmetic).  Bad arguments: SUMK_ERR_ARG, a message
 * naming the argument in sumk_last_error, nothing launched. */
int sumk_attn_strips_b16_sizes(int32_t n_seq, const int32_t* seq_off_host, int64_t* e_elems, int64_t* p16_elems);
int sumk_attn_strips_b16(int32_t backward, const void* A16, int32_t lda, const void* B16, int32_t ldb, const void* C16, int32_t ldc,
                         void* O16, int32_t ldo, float* E, void* P16, int32_t D, int32_t n_seq, const int32_t* seq_off_host,
                         float scale, int32_t ignore_self, int32_t aperture, float dropout_p, uint64_t seed, void* stream);
/* C(M,N) = A(M,K) * B(K,N) */
int sumk_gemm_nn(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, void* stream);
/* C(M,N) = A^T * B with A given as (K,M), B as (K,N) */
int sumk_gemm_tn(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, void* stream);

/* ------------------------------------------------------------------------------------------------ change points (KTS)
 * Kernel temporal segmentation (Potapov et al. 2014) of every video of a packed batch (csrc/kts.hip).  No reference counterpart: the
 * reference READS `change_points` / `n_frame_per_seg` (summarizer/utils/eval.py:74-94) that were prepared offline with KTS
 * (summarizer/datasets/README.md); these calls are that step, so scores become key shots for videos that come without the fields.
 * Per video of n = seq_off[v + 1] - seq_off[v] steps, with K = X X^T (exact fp32 MFMA) and everything behind it in float64:
 *   J[i,j]  = sum_{t=i..j} K[t,t] - (1 / (j - i + 1)) sum_{s,t=i..j} K[s,t]                       scatter of the segment i..j
 *   I[0,l]  = J[0,l-1] for lmin <= l < lmax (EXCLUSIVE upper bound: the original's quirk), 1e101 elsewhere
 *   I[k,l]  = min_{max(k lmin, l - lmax) <= t < l} I[k-1,t] + J[t,l-1],  p[k,l] = the SMALLEST minimising t        (cpd_nonlin)
 *   cost[k] = I[k,n] / n + (vmax k / (2 n)) (ln(n / k) + 1),  m_best = the SMALLEST minimising k; infinite scores never win   (cpd_auto)
 *   cps     = backtrack through p from (m_best, n): ascending step indices, each the first step of a new segment.
 * A video shorter than max_ncp + 1 steps is treated as max_ncp = n - 1 (n == 1: no change point).  Outputs (device): n_cps (n_seq) =
 * m_best; cps (n_seq, max_ncp), -1 behind n_cps[v]; scores (n_seq, max_ncp + 1) or NULL = I[k,n] for k <= n_cps[v], +inf where it
 * exceeds 1e99 and behind n_cps[v].  Limits: 1 <= n <= 16384 per video, D % 4 == 0, 1 <= lmin <= lmax, 0 <= max_ncp <= longest
 * video - 1; anything else -- a short workspace included -- returns SUMK_ERR_ARG and launches nothing.  One workgroup per video runs
 * the max_ncp dependent steps; ties resolve to the smallest index and nothing is accumulated with atomics: results are
 * bit-deterministic.  No host synchronisation inside the calls.
 * sumk_kts_workspace_bytes: pure host arithmetic (0 = bad arguments); the size serves all three calls.
 * sumk_kts_gram: the classic interface -- the caller's float64 kernel matrices, (n_v x n_v) blocks back to back, any kernel.
 * sumk_kts_gram_nonlin: cpd_nonlin itself -- the backtrack from row min(ncp, n - 1) with no penalty; scores = the whole row I[., n]. */
size_t sumk_kts_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t max_ncp);
int sumk_kts(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t max_ncp,
             int32_t lmin, int32_t lmax, double vmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
             size_t workspace_bytes, void* stream);
int sumk_kts_gram(const double* K, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t max_ncp,
                  int32_t lmin, int32_t lmax, double vmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
                  size_t workspace_bytes, void* stream);
int sumk_kts_gram_nonlin(const double* K, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t ncp,
                         int32_t lmin, int32_t lmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ change points, banded (long videos)
 * sumk_kts for videos past its 16384 steps, or long enough that one workgroup per video is the wrong shape (csrc/kts_banded.hip).  The
 * definition, the tie rules (smallest t, smallest k), the exclusive lmax of row 0 and the outputs (-1 behind n_cps[v], +inf where a score
 * exceeds 1e99 and behind n_cps[v]) are those of sumk_kts above.  Two things differ:
 *   storage  with B = min(lmax, n) only J[t, t .. t + B - 1] is built and kept per row t (pitch B), and the fp32 Gram only in 64-row strips
 *            of at most B + 63 columns from their own diagonal: the workspace is O(n B), not O(n^2), every offset 64-bit, p int32;
 *   the DP   row k is ONE launch over the end points l of all videos (lane = l, the window max(k lmin, l - lmax) <= t < l cut over the
 *            waves of a block, partial minima joined by an explicit (value, index) compare), rows with (k + 1) lmin > n are not launched,
 *            and one closing launch does penalty, arg-min, backtrack and scores.  Stream order is the only dependency between rows: no
 *            grid barrier, no cooperative launch, no spin-wait, no float atomics.  The call enqueues 6 + rows launches and never waits.
 * Inside the band every number comes from the arithmetic of the dense path in its order (same lean NT Gram launch and K loop, same
 * descending-s column sums, same 64-wide scans with carry, c = I[k-1,t] + J[t,l-1] under a strict < on ascending t), so for every input
 * both calls accept, n_cps, cps and the bits of scores EQUAL those of sumk_kts whatever lmax is; results are bit-deterministic.
 * Limits: 1 <= n <= 1048576 per video, at most 65535 videos, D % 4 == 0, 1 <= lmin <= lmax, 0 <= max_ncp <= longest video - 1; anything
 * else -- a short workspace included -- returns SUMK_ERR_ARG, sets sumk_last_error and launches nothing.
 * sumk_kts_banded_workspace_bytes: pure host arithmetic (0 = bad arguments): about n (8 B + 4 (B + 63) + 4 max_ncp) bytes per video. */
size_t sumk_kts_banded_workspace_bytes(int32_t D, int32_t n_seq, const int32_t* seq_off_host, int32_t max_ncp, int32_t lmax);
int sumk_kts_banded(const float* x, int32_t D, int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev, int32_t max_ncp,
                    int32_t lmin, int32_t lmax, double vmax, int32_t* n_cps, int32_t* cps, double* scores, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ shot selection
 * HOST function (no GPU work).  Replaces knapsack_ortools (summarizer/utils/knapsack.py:5-23): maximise
 * sum(values[i]) subject to sum(weights[i]) <= capacity; selected[i] = 1 for chosen items.  values/weights are the
 * integers the reference builds (knapsack.py:11-15: int(score*1000), int(n_frames_of_segment)). */
int sumk_knapsack_dp(const int64_t* values, const int64_t* weights, int32_t n_items, int64_t capacity,
                     uint8_t* selected);

/* HOST function, natively threaded (no GPU work): the evaluation tail of `Trainer.test` for a batch of videos --
 * upsample (summarizer/utils/eval.py:15-35), generate_summary (eval.py:74-123), evaluate_summary (eval.py:125-165) and
 * evaluate_scores with metric "spearmanr" (eval.py:49-72).  Machine summaries and F-scores are bit-identical to the numpy
 * implementation (numpy's float32 pairwise summation is reproduced); the rank correlation is float64, equal to ~1e-15. */
typedef struct sumk_eval_video {
  const float* scores; int32_t n_steps;        /* in: per-step importance scores                                      */
  const int32_t* picks; int32_t n_picks;       /* in: positions of the sampled frames                                 */
  int32_t n_frames;
  const int32_t* cps; const int32_t* nfps; int32_t n_segs;   /* in: change points (n_segs,2), frames per segment; n_segs 0: skip summary */
  const float* user_summary; int32_t n_users;  /* in: (n_users, n_frames), > 0 means selected                         */
  const double* user_ranks;                    /* in: (n_users, n_frames) average ranks of -user_scores, or NULL: skip correlation */
  float* machine_summary;                      /* out (optional): (sum nfps) 0/1 floats                               */
  int32_t summary_len;                         /* out: sum nfps                                                        */
  double corr, f_avg, f_max;                   /* out: mean Spearman over annotators; mean / max F-score (NaN if skipped) */
  const float* seg_means;                      /* in (optional): (n_segs) float32 segment means already taken on the DEVICE (sumk_eval_device):
                                                  upsampling, the means and the correlation are then skipped (corr is left as given) */
} sumk_eval_video;
/* method: 0 = knapsack (sumk_knapsack_dp), 1 = rank.  n_threads <= 0: min(16, hardware threads). */
int sumk_eval_videos(sumk_eval_video* videos, int32_t n_videos, double proportion, int32_t method, int32_t n_threads);

/* Device-side part of the same tail: the batch's scores stay in HBM; one launch (a block per video)
 * expands them to frame scores, takes the float32 segment means of eval.py:91-94 (numpy's pairwise summation reproduced, so
 * `int(mean * 1000)` and with it the key-shot selection are unchanged) and the mean Spearman correlation of eval.py:49-72.
 * The caller copies seg_means / corr back (one small D2H) and finishes on the host with sumk_eval_videos(seg_means given).
 * All pointers inside the descriptors are DEVICE pointers; picks must be ascending, n_picks <= 4096, n_users <= 32.
 * user_mean[u] / user_ssq[u] = mean and sum of squared deviations of annotator u's ranks (constants of the video). */
typedef struct sumk_eval_dev_video {
  const int32_t* picks; int32_t n_picks; int32_t n_frames; int32_t n_steps;
  int32_t row0;                                /* first row of this video in the packed score vector                   */
  int32_t frame0;                              /* offset of this video's frames in frame_scratch                       */
  const int32_t* cps; int32_t n_segs; int32_t seg0;   /* (n_segs,2) change points; offset of its segments in seg_means */
  const double* user_ranks; const double* user_mean; const double* user_ssq; int32_t n_users;   /* NULL / 0: no correlation (NaN) */
} sumk_eval_dev_video;
int sumk_eval_device(const float* scores_dev, const sumk_eval_dev_video* videos_dev, int32_t n_videos, float* frame_scratch_dev,
                     float* seg_means_dev, double* corr_dev, void* stream);
/* The same tail as two calls, so that the host's key-shot selection (which needs the segment means only) runs UNDER the correlation:
 * _segments = upsample + segment means (a block per video); _spearman = the correlation spread over 8 blocks per video + a final kernel
 * that adds their partial sums in order (scratch: sumk_eval_device_spearman_scratch_bytes(n_videos), 8-byte aligned).  The same
 * descriptors; results equal sumk_eval_device's (segment means bit for bit, correlations to float64 re-association). */
int sumk_eval_device_segments(const float* scores_dev, const sumk_eval_dev_video* videos_dev, int32_t n_videos, float* frame_scratch_dev,
                              float* seg_means_dev, void* stream);
size_t sumk_eval_device_spearman_scratch_bytes(int32_t n_videos);
int sumk_eval_device_spearman(const float* scores_dev, const sumk_eval_dev_video* videos_dev, int32_t n_videos, double* scratch_dev,
                              double* corr_dev, void* stream);

/* Kendall's tau-b instead of Spearman's rho (evaluate_scores with metric "kendalltau", eval.py:56-59 = scipy.stats.kendalltau, variant b,
 * of the two rank vectors), per (video, annotator) from integer pair counts, n = n_frames:
 *   tot = n (n - 1) / 2;  xtie / ytie / ntie = sum t (t - 1) / 2 over the tie groups of the machine frame scores / the annotator's scores /
 *   the (x, y) pairs;  dis = discordant pairs;  cmd = tot - xtie - ytie + ntie - 2 dis;
 *   tau = cmd / sqrt(tot - xtie) / sqrt(tot - ytie) (float64, in this order), clamped to [-1, 1]; NaN when xtie == tot or ytie == tot.
 * A video's value is the mean over its annotators in numpy's summation order (NaN if any annotator's is).  O(n log n) everywhere.
 *
 * HOST, threaded like sumk_eval_videos: upsample + tau-b against user_ranks for every video; writes .corr only (NaN without user_ranks).
 * counts (optional): {cmd, xtie, ytie, ntie} per (video, annotator), the annotators of video i after those of videos 0 .. i - 1. */
int sumk_eval_videos_kendall(sumk_eval_video* videos, int32_t n_videos, int64_t* counts, int32_t n_threads);
/* DEVICE: takes the place of sumk_eval_device_spearman behind sumk_eval_device_segments, on the same descriptors plus one
 * sumk_eval_dev_kendall per video (a parallel array).  One workgroup per (video, annotator) sorts the video's frame keys in LDS: on top of
 * the limits of sumk_eval_dev_video, n_frames <= 16384.  A descriptor past a limit gets NaN (and -1 in its counts) and nothing else is
 * touched.  scratch: sumk_eval_device_kendall_scratch_bytes(n_videos, total frames of the batch) bytes, 8-byte aligned.
 * counts_dev (optional): 4 int64 {cmd, xtie, ytie, ntie} per annotator, annotator u of a video at counts_dev[4 * (counts0 + u)].
 * Results equal the host function's bit for bit (the same integers, the same float64 operations). */
typedef struct sumk_eval_dev_kendall {
  const int32_t* y_dense;                      /* (n_users, n_frames) dense ranks of each annotator's scores: 0-based, ascending with the score, equal scores share one */
  const int64_t* ytie;                         /* (n_users) tied pairs of each annotator's scores                                              */
  int64_t counts0;                             /* first annotator slot of this video in counts_dev                                             */
} sumk_eval_dev_kendall;
size_t sumk_eval_device_kendall_scratch_bytes(int32_t n_videos, int64_t total_frames);
int sumk_eval_device_kendall(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_kendall* kendall_dev,
                             int32_t n_videos, void* scratch_dev, double* corr_dev, int64_t* counts_dev, void* stream);

/* DEVICE: key-shot selection, summary expansion and F-scores behind sumk_eval_device_segments (csrc/evalselect.hip) -- what
 * sumk_eval_videos(seg_means given) does on the host, with the segment means where the device left them.  One launch, one workgroup per
 * video, no atomics, no host synchronisation (capturable into a HIP graph).  Results equal the host's bit for bit: the values are
 * (int64_t)((double)seg_mean * 1000.0) and the weights nfps[s]; method 0 selects exactly the set of sumk_knapsack_dp (its last-improver
 * tie rule and its quirks: item 0 is taken when nothing improved the remaining capacity and it fits; nothing is taken when item 0 is too
 * heavy), method 1 the set of the rank walk (descending score, the larger index first among equals, strict total + nfps < capacity); the
 * summary holds nfps[s] entries of selected[s] per segment; F-scores follow evaluate_summary (float32, float64 when summary_len <
 * n_frames) with the mean over annotators in numpy's pairwise order.
 * Per video: seg_means (n_segs) float32 and nfps (n_segs) int32 on the device; capacity = floor((double)n_frames * proportion) and
 * summary_len = sum(nfps), both computed by the caller; summary0 / sel0 = the video's offsets in machine_summary_dev / selected_dev;
 * user_mask (n_users, n_frames) uint8 = the annotators' summaries binarised with > 0 (NULL or n_users 0: F-scores are NaN); method is
 * one value per call.  Outputs (device): machine_summary (summary_total) float32 0 / 1, selected (selected_total) uint8, f_avg / f_max
 * (n_videos) float64, status (n_videos) int32.
 * Limits: 1 <= n_segs <= SUMK_SELECT_MAX_SEGS, 0 <= capacity <= SUMK_SELECT_MAX_CAPACITY (54 000 frames at proportion 0.15), n_users <=
 * SUMK_SELECT_MAX_USERS, 1 <= n_frames <= 2^24.  The profit rows of the knapsack live in LDS up to capacity SUMK_SELECT_LDS_CAPACITY and in
 * the workspace above it.  Everything the host can see -- these limits, null pointers, offsets outside the outputs, a short workspace --
 * returns SUMK_ERR_ARG and launches nothing: the entry point reads videos_host, the host copy of the descriptor array videos_dev.
 * status: 0 fine; 1 a segment mean is not finite or exceeds 1e12 in magnitude (the host's cast to int64 is undefined there); 2 the
 * positive values that fit the capacity sum to 2^31 or more (the int32 profit rows would not hold the host's int64 result: means whose
 * thousandfolds add up past 2.1e9); 3 a negative nfps, or nfps that do not sum to summary_len; 4 a device descriptor past the limits.
 * A video with a nonzero status gets an all-zero summary and selection (status 4: neither is written) and NaN F-scores; the other videos
 * of the call are unaffected and nothing is written out of bounds.
 * workspace: sumk_eval_device_select_workspace_bytes(n_videos, largest n_segs, largest capacity) bytes, 8-byte aligned, contents
 * irrelevant; pure host arithmetic, 0 = bad arguments. */
#define SUMK_SELECT_MAX_SEGS 1024
#define SUMK_SELECT_MAX_CAPACITY 8191
#define SUMK_SELECT_LDS_CAPACITY 4095
#define SUMK_SELECT_MAX_USERS 32
typedef struct sumk_eval_dev_select {
  const float* seg_means; const int32_t* nfps;
  int32_t n_segs; int32_t n_frames; int32_t capacity; int32_t summary_len;
  int64_t summary0; int64_t sel0;
  const uint8_t* user_mask; int32_t n_users;
  int32_t method;                              /* 0 = knapsack, 1 = rank                                                */
} sumk_eval_dev_select;
size_t sumk_eval_device_select_workspace_bytes(int32_t n_videos, int32_t max_n_segs, int32_t max_capacity);
int sumk_eval_device_select(const sumk_eval_dev_select* videos_dev, const sumk_eval_dev_select* videos_host, int32_t n_videos,
                            float* machine_summary_dev, int64_t summary_total, uint8_t* selected_dev, int64_t selected_total,
                            double* f_avg_dev, double* f_max_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes,
                            void* stream);

/* DEVICE, long videos (csrc/evallong.hip): the same two steps without the per-video LDS tables of the calls above, for what
 * sumk_kts_banded segments.  Neither uses a cooperative launch or a flag polled across workgroups: every launch ends by itself, the
 * work of a video is spread over the chip, and both can be captured into a HIP graph.
 *
 * sumk_eval_device_segments_long: sumk_eval_device_segments on the same descriptors, results equal bit for bit wherever both accept the
 * input.  Upsampling is frame-centric on a grid over (frame chunks, videos): frame f takes the score of the last pick interval i with
 * picks[i] <= f by binary search (0 for i >= n_steps and for frames in front of the first pick) -- for ascending picks, duplicates
 * allowed, the array the in-order interval loop writes.  A segment mean is one workgroup per (video, segment): numpy's float32 sum -- up to 8192 frames one
 * pairwise tree, cut at depth 8, a subtree per thread, joined in tree order; past that the trees of 8192-frame blocks added in order --
 * then one division; empty segments give 0.
 * Limits: 1 <= n_picks <= SUMK_SEGMENTS_LONG_MAX_PICKS (the cap of sumk_kts_banded), 1 <= n_frames <= SUMK_SEGMENTS_LONG_MAX_FRAMES,
 * n_segs >= 0, n_videos <= 65535; user_* are not read.  videos_host is the host copy of videos_dev: a video past a limit returns
 * SUMK_ERR_ARG and launches nothing.  A device descriptor that disagrees with it and is past a limit gets NaN segment means. */
#define SUMK_SEGMENTS_LONG_MAX_PICKS 1048576
#define SUMK_SEGMENTS_LONG_MAX_FRAMES 16777216
int sumk_eval_device_segments_long(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host,
                                   int32_t n_videos, float* frame_scratch_dev, float* seg_means_dev, void* stream);
/* sumk_eval_device_select_long: sumk_eval_device_select on the same descriptors, outputs and status codes, for any frame budget:
 * 1 <= n_segs <= SUMK_SELECT_MAX_SEGS, 0 <= capacity <= SUMK_SELECT_LONG_MAX_CAPACITY, n_users <= SUMK_SELECT_MAX_USERS, 1 <= n_frames <=
 * 2^24.  Results equal sumk_eval_device_select's and the host tail's bit for bit.  Launches: a prologue (one workgroup per video: the
 * integers, the items of the knapsack's pass, the status); method 0: one launch per item position j = 0 .. largest n_segs of the call
 * - 1 on a grid over (SUMK_SELECT_LONG_CHUNK capacities, videos), each reading one int32 profit row of the workspace and writing the
 * other plus one 64-bit word of improvement bits per wave -- a block whose video has fewer items in its pass, a nonzero status or
 * capacity 0 exits at once; the backtrack (method 1: the rank walk) per video; summary expansion and the annotators' int32 counts over
 * (frame chunks, videos); a last launch that adds the counts and takes the F-scores.
 * A device descriptor past the limits, past the call's largest n_segs / capacity / n_frames as the host copy has them, or with offsets
 * outside the outputs gets status 4 and nothing else of it is written.
 * workspace: sumk_eval_device_select_long_workspace_bytes(n_videos, largest n_segs, largest capacity) bytes, 8-byte aligned, contents
 * irrelevant; pure host arithmetic, 0 = bad arguments.  Per video, each part rounded up to 256 bytes: n_segs x ceil((capacity + 1) / 64)
 * 64-bit words of improvement bits; two rows of capacity + 1 int32; 5 n_segs + 9 int32 of item tables; SUMK_SELECT_LONG_FRAME_CHUNKS x
 * (2 SUMK_SELECT_MAX_USERS + 1) int32 of partial counts.  The bits are what grows: n_segs x capacity / 8 bytes. */
#define SUMK_SELECT_LONG_MAX_CAPACITY 16777216
#define SUMK_SELECT_LONG_CHUNK 2048
#define SUMK_SELECT_LONG_FRAME_CHUNKS 64
size_t sumk_eval_device_select_long_workspace_bytes(int32_t n_videos, int32_t max_n_segs, int32_t max_capacity);
int sumk_eval_device_select_long(const sumk_eval_dev_select* videos_dev, const sumk_eval_dev_select* videos_host, int32_t n_videos,
                                 float* machine_summary_dev, int64_t summary_total, uint8_t* selected_dev, int64_t selected_total,
                                 double* f_avg_dev, double* f_max_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* Rank correlation for long videos (csrc/evalcorr_long.hip): sumk_eval_device_spearman_long and sumk_eval_device_kendall_long take the
 * place of sumk_eval_device_spearman / sumk_eval_device_kendall behind sumk_eval_device_segments_long, on the same descriptors
 * (sumk_eval_dev_video, plus one sumk_eval_dev_kendall per video for Kendall) and with the same results: Kendall's tau, its mean and the
 * counts {cmd, xtie, ytie, ntie} bit for bit (integers, then kendall_tau_b and numpy's summation order); Spearman to float64
 * re-association (the ranks are the same values; the sum of squared rank deviations is taken over the groups, the cross terms over
 * min(256, ceil(n_frames / 4096)) chunks of the video's frames, added in chunk order -- a video's result does not depend on the other
 * videos of the call).  NaN where the block kernels give NaN: no annotators, Spearman without user_ranks, a constant side.
 * Limits: 1 <= n_picks <= SUMK_SEGMENTS_LONG_MAX_PICKS, 1 <= n_frames <= SUMK_SEGMENTS_LONG_MAX_FRAMES, n_users <= 32, n_videos <= 65535;
 * picks ascend.  Everything the host can see -- these limits in videos_host (the host copy of videos_dev), a null pointer, a short
 * workspace -- returns SUMK_ERR_ARG and launches nothing.  A device descriptor that disagrees with the host copy and is past a limit, or
 * past the call's largest n_picks / n_frames / n_users as the host copy has them, gets NaN (Kendall: and -1 in its counts); nothing is
 * written out of bounds and the other videos are unaffected.
 * How: the groups of a video (its pick intervals plus the frames no interval covers) are sorted by value with a chip-wide stable merge
 * sort -- tiles of SUMK_CORR_LONG_TILE keys in LDS, then one launch per merge level over two buffers, every element placed by one binary
 * search in the sibling run; prefix sums over the sorted groups give every rank and tie count as integers.  Kendall sorts the 64-bit
 * frame keys (dense x rank << 24 | y_dense) of every (video, annotator) with the same sort, then their y parts with its inversion count
 * on.  No cooperative launch, no flag polled across workgroups, no float atomics; the launches depend on videos_host only, so a call
 * captures into a HIP graph.
 * workspace: sumk_eval_device_{spearman,kendall}_long_workspace_bytes(videos_host, n_videos) bytes, 8-byte aligned, contents irrelevant;
 * pure host arithmetic, 0 = bad arguments.  With G = sum(n_picks + 1), B = sum(ceil((n_picks + 1) / 1024)), U = sum(max(n_users, 0)),
 * UF = sum(max(n_users, 0) x n_frames) and C = sum(min(256, ceil(n_frames / 4096))) over the videos, each part rounded up to 256 bytes:
 *   both      72 n_videos (headers) + 8 G + 8 G (group keys, two buffers) + 4 G + 4 G (prefix sums) + 8 B (scan blocks)
 *   Spearman  + 8 G (ranks) + 8 x 33 C (partial sums)
 *   Kendall   + 4 G (dense x ranks) + 8 UF + 8 UF (frame keys, two buffers: 16 bytes per annotator and frame) + 8 (2 U + n_videos) (counters) */
#define SUMK_CORR_LONG_TILE 2048   /* keys one workgroup sorts in LDS before the global merge levels; exported so tests can sit on its edges */
size_t sumk_eval_device_spearman_long_workspace_bytes(const sumk_eval_dev_video* videos_host, int32_t n_videos);
int sumk_eval_device_spearman_long(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host,
                                   int32_t n_videos, void* workspace, size_t workspace_bytes, double* corr_dev, void* stream);
size_t sumk_eval_device_kendall_long_workspace_bytes(const sumk_eval_dev_video* videos_host, int32_t n_videos);
int sumk_eval_device_kendall_long(const float* scores_dev, const sumk_eval_dev_video* videos_dev, const sumk_eval_dev_video* videos_host,
                                  const sumk_eval_dev_kendall* kendall_dev, int32_t n_videos, void* workspace, size_t workspace_bytes,
                                  double* corr_dev, int64_t* counts_dev, void* stream);
/* DEVICE: (n_cps, cps) of sumk_kts -> the change points the evaluation tail reads, at a fixed pitch of max_ncp + 1 segments per video, so
 * that n_segs stays a host-known bound: change_points (n_seq, max_ncp + 1, 2) and nfps (n_seq, max_ncp + 1) int32.  Segment s <= n_cps[v]
 * is [0 | frame(cps[s - 1]), frame(cps[s]) - 1 | n_frames[v] - 1] with frame(c) = picks_dev[v][c] (picks_dev, or an entry of it, NULL: c
 * itself) and nfps = its length; the segments behind are EMPTY: (n_frames, n_frames - 1), nfps 0 -- mean 0 from the segments kernel, never
 * an improvement of a knapsack capacity, no frames in rank mode: the summary equals the unpadded one. */
int sumk_kts_segments(const int32_t* n_cps_dev, const int32_t* cps_dev, int32_t n_seq, int32_t max_ncp, const int32_t* seq_off_dev,
                      const int32_t* const* picks_dev, const int32_t* n_frames_dev, int32_t* change_points_dev, int32_t* nfps_dev,
                      void* stream);

/* ------------------------------------------------------------------------------------------------ dataset records from raw annotations
 * DEVICE: the frame-level arithmetic that turns a video's raw annotations into the fields a trainer reads (csrc/annotate.hip).  No
 * reference counterpart: the reference READS gtscore / user_scores / user_summary / gtsummary that other projects' code prepared offline
 * (summarizer/datasets/README.md:50-74); sumk_annotate is that step, in front of sumk_eval_device_segments and sumk_eval_device_select,
 * which make the summaries from what it leaves in HBM (summarizer_amd/utils/annotate.py: annotate_batch).
 * Per video: anno (n_users, n_frames) float32, picks (n_picks) int32 ascending inside 0 .. n_frames - 1, cps (n_segs, 2) int32 -- all
 * DEVICE pointers.  All arithmetic is float32, in exactly this order (the unit is compiled without FMA contraction):
 *   protocol SUMK_ANNOTATE_SCORES (TVSum style: grades in [lo, hi]):
 *     user[u][f]   = (anno[u][f] - lo) / (hi - lo)                                                  -> the record's user_scores
 *     consensus[f] = (((anno[0][f] + anno[1][f]) + ...) + anno[U-1][f]) / (float)U                  (sequential in u, from 0.f)
 *     g[t]         = consensus[picks[t]];  gtscore[t] = (g[t] - min g) / (max g - min g), all 0 when max g == min g
 *     seg_means[u][s] = pairwise_sum(user[u][start_s .. end_s]) / (float)count_s, 0 for an empty segment (numpy's float32 pairwise tree,
 *                    the one of sumk_eval_device_segments): the knapsack / rank values of annotator u's own summary
 *   protocol SUMK_ANNOTATE_SUMMARIES (SumMe style: any value > 0 means selected):
 *     user[u][f]   = anno[u][f] > 0 ? 1 : 0                                                         -> the record's user_summary
 *     consensus[f] = (float)count_u(anno[u][f] > 0) / (float)U;  gtscore[t] = consensus[picks[t]] (not normalised); no seg_means.
 * Offsets (in elements) place the video in the caller's outputs: user0 its (n_users, n_frames) block in user_dev, frame0 its n_frames
 * entries in consensus_dev, pick0 its n_picks entries in gtscore_dev (and in the gtsummary of sumk_annotate_gtsummary), seg0 its
 * (n_users, n_segs) block in seg_means_dev, gtsum0 its n_frames entries in the frame summary sumk_annotate_gtsummary reads.
 * summary_len = sum of the frames per segment, computed by the caller: the segments must tile the frames (summary_len == n_frames).
 * Limits, those of the kernels this chains into: 1 <= n_users <= SUMK_SELECT_MAX_USERS, 1 <= n_picks <= 4095, 1 <= n_segs <=
 * SUMK_SELECT_MAX_SEGS, 1 <= n_frames <= 2^24, hi > lo (both finite), n_videos <= 65535 and ceil(longest video / 256) x n_videos < 2^24 (one
 * launch covers every frame of the batch), reserved == 0.  Everything the host can see -- these limits,
 * null pointers, blocks outside the outputs -- returns SUMK_ERR_ARG and launches nothing: the entry reads videos_host, the host copy of
 * videos_dev.  On the device every index read from picks or cps is clamped to the video, and a device descriptor past the limits is
 * skipped: nothing is read or written out of bounds.  Two launches (one pass over the annotations; one workgroup per video for the
 * reduction and one thread per (annotator, segment) mean), no atomics, no cooperative launch, no host synchronisation: capturable.
 * sumk_annotate_gtsummary: gtsummary[pick0 + t] = frame_summary[gtsum0 + picks[t]] -- the key-shot summary of gtscore that
 * sumk_eval_device_select expanded to frames, sampled back at the picks (the record's gtsummary).  Same descriptors, same checks. */
#define SUMK_ANNOTATE_SCORES 0
#define SUMK_ANNOTATE_SUMMARIES 1
#define SUMK_ANNOTATE_MAX_PICKS 4095
typedef struct sumk_annotate_video {
  const float* anno; const int32_t* picks; const int32_t* cps;
  int32_t n_users; int32_t n_frames; int32_t n_picks; int32_t n_segs;
  int32_t summary_len; int32_t reserved;       /* reserved: 0                                                            */
  int64_t user0; int64_t frame0; int64_t pick0; int64_t seg0; int64_t gtsum0;
} sumk_annotate_video;
int sumk_annotate(const sumk_annotate_video* videos_dev, const sumk_annotate_video* videos_host, int32_t n_videos, int32_t protocol,
                  float lo, float hi, float* user_dev, int64_t user_total, float* consensus_dev, int64_t frame_total, float* gtscore_dev,
                  int64_t pick_total, float* seg_means_dev, int64_t seg_total, void* stream);
int sumk_annotate_gtsummary(const sumk_annotate_video* videos_dev, const sumk_annotate_video* videos_host, int32_t n_videos,
                            const float* frame_summary_dev, int64_t frame_summary_total, float* gtsummary_dev, int64_t pick_total,
                            void* stream);

/* ------------------------------------------------------------------------------------------------ inter-annotator agreement
 * DEVICE: how well the annotators of a video agree with each other under the two metrics of the evaluation tail (csrc/agreement.hip;
 * summarizer_amd/utils/agreement.py chains the three calls; the specification is tests/agreement_ref.py, bit for bit).
 * Per video: user_summary (n_sum, n_frames) float32, > 0 = selected, and / or user_scores (n_sc, n_frames) float32, finite -- DEVICE
 * pointers, NULL with a count of 0.  Offsets (in elements) place the video in the caller's buffers: rank0 its (n_sc, n_frames) block of
 * ranks, row0 its n_sc per-row entries (ties, mean, ssq, corr_user), sum0 its n_sum entries of f_avg_user / f_max_user, f0 its
 * (n_sum, n_sum) block of F, c0 its (n_sc, n_sc) block of C (and 4 x that in counts).
 * sumk_rank_rows, one workgroup per row sorting kendall_float_key(x) in LDS (-0.0 and 0.0 are one value):
 *   avg_ranks  float64, 1-based average ranks of -x = scipy.stats.rankdata(-x)
 *   dense      int32, 0-based, ascending with the score, equal scores share one rank
 *   ties       int64, sum t (t - 1) / 2 over the groups of equal scores
 *   mean, ssq  float64 (n + 1) / 2 and sum (rank - mean)^2: multiples of 0.25 below 2^53, exact in any order
 * sumk_agreement_f, one workgroup per video, float32 as evaluate_summary(user_summary[a], user_summary[b:b+1]) (eval.py:125-165):
 *   F[a][b] = 2PR / (P + R), P = o / (sum_a + 1e-8), R = o / (sum_b + 1e-8), 0 when both are 0 -- the arithmetic of sumk_eval_device_select
 *   f_avg_user[a] / f_max_user[a] = float32 mean (numpy's pairwise order) / maximum over b != a in index order
 *   f_avg / f_max (per video) = float64 mean of those over a; all four NaN when n_sum < 2 (F is still written)
 * sumk_agreement_corr on the outputs of sumk_rank_rows:
 *   metric SUMK_AGREEMENT_SPEARMAN  C[a][b] = sum (r_a - mean)(r_b - mean) / sqrt(ssq_a ssq_b): NaN for a constant row
 *   metric SUMK_AGREEMENT_KENDALL   C[a][b] = tau-b of sumk_eval_device_kendall from integer pair counts, x = annotator a, y = annotator b;
 *                                   counts (optional) = {cmd, xtie, ytie, ntie} per entry of C
 *                                   A pair whose rows hold few distinct values (their product <= 1024: TVSum grades give 5 x 5) takes its
 *                                   counts from the rows' contingency table in LDS, every other pair from an LDS merge sort: the same integers.
 *   corr_user[a] = float64 mean over b != a, corr (per video) = float64 mean over a, numpy's pairwise order, NaN propagates; NaN when n_sc < 2
 * Limits: n_sum, n_sc <= SUMK_SELECT_MAX_USERS; 1 <= n_frames <= 2^24 for F and <= 16384 where n_sc > 0; n_videos <= 65535; reserved == 0.
 * Everything the host can see -- these limits, null pointers, blocks outside the buffers -- returns SUMK_ERR_ARG and launches nothing: the
 * entries read videos_host, the host copy of videos_dev.  A device descriptor past a limit gets NaN in its per-video results (NaN / -1 in
 * the scalars of a rank row) and nothing else is touched.  No atomics, no cooperative launch, no host synchronisation: capturable. */
#define SUMK_AGREEMENT_SPEARMAN 0
#define SUMK_AGREEMENT_KENDALL 1
#define SUMK_AGREEMENT_KENDALL_SORT 2          /* Kendall with every pair through the sort: what the tests hold the table path to     */
typedef struct sumk_agreement_video {
  const float* user_summary; const float* user_scores;
  int32_t n_frames; int32_t n_sum; int32_t n_sc; int32_t reserved;       /* reserved: 0                                        */
  int64_t rank0; int64_t row0; int64_t sum0; int64_t f0; int64_t c0;
} sumk_agreement_video;
int sumk_rank_rows(const sumk_agreement_video* videos_dev, const sumk_agreement_video* videos_host, int32_t n_videos, double* avg_ranks_dev,
                   int32_t* dense_ranks_dev, int64_t rank_total, int64_t* ties_dev, double* mean_dev, double* ssq_dev, int64_t row_total,
                   void* stream);
int sumk_agreement_f(const sumk_agreement_video* videos_dev, const sumk_agreement_video* videos_host, int32_t n_videos, float* F_dev,
                     int64_t f_total, float* f_avg_user_dev, float* f_max_user_dev, int64_t sum_total, double* f_avg_dev, double* f_max_dev,
                     void* stream);
int sumk_agreement_corr(const sumk_agreement_video* videos_dev, const sumk_agreement_video* videos_host, int32_t n_videos, int32_t metric,
                        const double* avg_ranks_dev, const int32_t* dense_ranks_dev, int64_t rank_total, const int64_t* ties_dev,
                        const double* ssq_dev, int64_t row_total, double* C_dev, int64_t c_total, int64_t* counts_dev,
                        double* corr_user_dev, double* corr_dev, void* stream);

/* ------------------------------------------------------------------------------------------------ data-parallel exchange (RCCL)
 * The gradient all-reduce of data-parallel training as a library call: SUM, in place, over one flat bucket, on the caller's
 * HIP stream (one collective per optimiser step; the reference has no distributed code).  Bootstrap:
 * rank 0 obtains a 128-byte id (sumk_comm_unique_id) and ships it to every rank by any channel it has; every rank then calls
 * sumk_comm_init with its rank -- the communicator binds the CURRENT HIP device.  dtype: 0 = fp32, 1 = bf16 (the
 * mixed-precision mode's gradient bucket).  RCCL is dlopen'ed on first use (never linked): single-GPU users never load it.
 * summarizer_amd/training.py uses torch.distributed by default and this path under SUMK_RCCL_DIRECT=1. */
int sumk_comm_unique_id(uint8_t* id128);
int sumk_comm_init(const uint8_t* id128, int32_t rank, int32_t world, void** comm_out);
int sumk_allreduce_flat(void* comm, void* buf, int64_t n, int32_t dtype, void* stream);
int sumk_comm_destroy(void* comm);

/* ------------------------------------------------------------------------------------------------ feature ingest (host)
 * Packs the (n_rows[i], D) fp32 feature matrices srcs[i] back to back into dst (normally a pinned staging buffer that ONE
 * H2D copy then ships) with a pool of memcpy threads; replaces the per-video host->device uploads of the reference's loops
 * (summarizer/models/__init__.py:47-51, vasnet.py:194-205, dsn.py:98-110).  n_threads <= 0: min(16, hardware threads). */
int sumk_pack_rows(float* dst, const float* const* srcs, const int32_t* n_rows, int32_t n_videos, int32_t D, int32_t n_threads);
/* The same packing with fp32 -> bf16 (round to nearest even, NaN kept) folded into the copy: half the staging and H2D bytes for
 * link-bound hosts ("on-the-fly bf16 conversion").  LOSSY -- the scorer then sees bf16(features);
 * the device side widens with sumk_cast_bf16_f32.  Opt-in: summarizer_amd.ingest.StreamingScorer(stage_dtype="bf16"). */
int sumk_pack_rows_bf16(uint16_t* dst_bf16, const float* const* srcs, const int32_t* n_rows, int32_t n_videos, int32_t D, int32_t n_threads);

/* Per-kernel timing for bench.py's roofline object: launches tagged t are bracketed with hipEvents ON THE LAUNCH STREAM while
 * bit t of the mask passed to sumk_prof_enable is set (0 = off).  sumk_prof_read synchronises and returns the sums. */
#define SUMK_PROF_GEMM_QKV 0
#define SUMK_PROF_GEMM_ALL 1
#define SUMK_PROF_LSTM_REC 2
#define SUMK_PROF_GEMM_QKT 3     /* per-video Q.K^T launches of sumk_vasnet_forward                     */
#define SUMK_PROF_GEMM_PV 4      /* per-video alpha.V launches                                          */
#define SUMK_PROF_GEMM_OPROJ 5   /* output projection (+ residual)                                      */
#define SUMK_PROF_GEMM_K1 6      /* k1 (+ bias, ReLU)                                                   */
#define SUMK_PROF_BAND_SOFTMAX 7 /* band softmax launch of sumk_attn_band (its two products: QKT and PV above) */
/* the seven launches of the attention backward on the band (sumk_attn_band_backward), in launch order */
#define SUMK_PROF_BAND_BWD_TRANSPOSE_P 8   /* transpose(dropout(alpha))   */
#define SUMK_PROF_BAND_BWD_DV 9            /* dV = alphaD^T dCTX          */
#define SUMK_PROF_BAND_BWD_DP 10           /* dAlphaD = dCTX V^T          */
#define SUMK_PROF_BAND_BWD_SOFTMAX 11      /* softmax backward            */
#define SUMK_PROF_BAND_BWD_DQ 12           /* dQ = dLogits K              */
#define SUMK_PROF_BAND_BWD_TRANSPOSE_S 13  /* transpose(dLogits)          */
#define SUMK_PROF_BAND_BWD_DK 14           /* dK = dLogits^T Q            */
/* the launches of sumk_dsn_reward_stream (csrc/reward_stream.hip) */
#define SUMK_PROF_REWARD_STREAM_PREP 15    /* descriptors + pick bits               */
#define SUMK_PROF_REWARD_STREAM_NORM 16    /* squared norms: the diagonal Gram tiles */
#define SUMK_PROF_REWARD_STREAM_PASS 17    /* the streaming passes (one per chunk)  */
#define SUMK_PROF_REWARD_STREAM_ROWS 18    /* splits and rows joined per row block  */
#define SUMK_PROF_REWARD_STREAM_JOIN 19    /* per (episode, video): the reward      */
/* the Transformer scorer's attention, per layer: the three launches of the dense core (logits, softmax, context: csrc/transformer.hip
 * tf_attn_core_fwd) and the one launch of the stream form (csrc/attn_stream.hip, without its descriptor setup) */
#define SUMK_PROF_TF_ATTN_DENSE 20
#define SUMK_PROF_ATTN_STREAM 21
/* the stream form under training: the training-forward launch (csrc/attn_stream.hip with the statistic and the dropout), and the three
 * launches of its backward one by one (csrc/attn_stream_bwd.hip) */
#define SUMK_PROF_ATTN_STREAM_TRAIN 22
#define SUMK_PROF_ATTN_STREAM_BWD_DELTA 23
#define SUMK_PROF_ATTN_STREAM_BWD_DQ 24
#define SUMK_PROF_ATTN_STREAM_BWD_DKV 25
/* the stream form in bf16x3 (csrc/attn_stream_split.hip): the pass that splits Q, K, V into bf16 planes, and the attention launch */
#define SUMK_PROF_ATTN_STREAM_SPLIT_PLANES 26
#define SUMK_PROF_ATTN_STREAM_SPLIT 27
/* the bf16x3 stream form under training: the backward's split pass (Q, K, V, dctx -> planes), the training-forward launch
 * (csrc/attn_stream_split.hip with the statistic and the dropout; its own split pass keeps tag 26), and the two passes of the backward
 * (csrc/attn_stream_split_bwd.hip); its delta launch keeps tag 23 */
#define SUMK_PROF_ATTN_STREAM_SPLIT_BWD_PLANES 28
#define SUMK_PROF_ATTN_STREAM_SPLIT_TRAIN 29
#define SUMK_PROF_ATTN_STREAM_SPLIT_BWD_DQ 30
#define SUMK_PROF_ATTN_STREAM_SPLIT_BWD_DKV 31
#define SUMK_PROF_NTAGS 32
/* The small-batch GEMM form by itself (tests, probes): C = epilogue(A . B) for ONE exact-fp32 problem on 64x64 tiles whose K is cut
 * into `slices` (1 .. 8) slices INSIDE the launch -- every (tile, slice) block stores a partial tile, the last one to arrive adds
 * them in slice order and runs the epilogue (csrc/gemm_lean.hip, SK instances; what sumk_vasnet_forward / _backward launch for batches
 * of <= 1024 frames).  layout 0 NT (A (M,K), B (N,K)), 1 NN (B (K,N)), 2 TN (A (K,M), B (K,N)); epilogue 0 C = alpha acc, 1 acc + R,
 * 2 relu(acc + bias[col]), 4 C += alpha acc.  workspace: sumk_gemm_splitk_workspace_bytes(M, N, slices), 256-byte aligned. */
size_t sumk_gemm_splitk_workspace_bytes(int32_t M, int32_t N, int32_t slices);
int sumk_gemm_splitk(int32_t layout, const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb,
                     int32_t ldc, int32_t slices, int32_t epilogue, const float* R, int32_t ldr, const float* bias, float alpha,
                     void* workspace, size_t workspace_bytes, void* stream);
int sumk_prof_enable(int32_t tag_mask);
int sumk_prof_read(int32_t tag, double* total_ms, int64_t* launches, int32_t reset);

/* Measurement utility (no reference counterpart; bench.py's `mfma_sustained`): the rate the matrix pipes of the current device SUSTAIN with nothing but
 * MFMAs in flight -- one workgroup of eight waves per CU, four independent accumulators per wave, operands in registers, no memory traffic.  One warm-up
 * launch, one timed launch of `iters` x 16 MFMAs per wave (HIP events on `stream`; synchronises).  kind 0: v_mfma_f32_32x32x16_bf16, 1:
 * v_mfma_f32_32x32x2_f32, 2: v_mfma_f32_16x16x32_bf16; + 4: every MFMA of an iteration reads its own pseudo-random operand registers (the operand buses
 * toggle as under real data: the rate a real kernel can hope for) instead of one constant pair.  *tflops = dense TFLOP/s over the whole chip, *seconds
 * (may be null) = the timed launch. */
int sumk_probe_mfma_rate(int32_t kind, int32_t iters, double* tflops, double* seconds, void* stream);

/* ------------------------------------------------------------------------------------------------ Transformer stacks (SumGAN-Att)
 * The encoder and decoder stacks of the reference's SumGAN-Att (summarizer/models/sumgan_att.py:20-80) on the exact-fp32 path:
 * stock post-norm nn.TransformerEncoderLayer / nn.TransformerDecoderLayer (ReLU, dim_feedforward F, no masks), weights as torch
 * stores them.  Dropout: opts->layer_dropout_p at every site torch has one, deterministic hash masks of (opts->seed, site,
 * element); opts->layer_eps is the eps of the layers' norms, opts->final_eps that of the encoder's optional final norm;
 * opts->precision must be SUMK_PRECISION_FP32 and opts->wplanes NULL.  Gradients are ACCUMULATED into the grad structs. */
size_t sumk_tf_encoder_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                       const int32_t* seq_off_host, int32_t training);
/* x (n_rows,D) packed -> hidden (n_rows,D): n_layers encoder layers, then LayerNorm(norm_w, norm_b) when norm_w is non-NULL */
int sumk_tf_encoder_forward(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                            const int32_t* seq_off_host, const int32_t* seq_off_dev, const sumk_tf_layer_weights* layers,
                            const float* norm_w, const float* norm_b, const sumk_tf_opts* opts, float* hidden, void* workspace,
                            size_t workspace_bytes, int32_t training, void* stream);
/* Backward of sum(dhidden * hidden) after a training-mode forward on the same workspace: dx (if non-NULL) is written; the
 * final norm's gradients go to dnorm_w / dnorm_b (both non-NULL when the forward had the norm). */
int sumk_tf_encoder_backward(const float* x, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                             const int32_t* seq_off_host, const int32_t* seq_off_dev, const sumk_tf_layer_weights* layers,
                             const float* norm_w, const float* norm_b, const sumk_tf_opts* opts, const float* dhidden,
                             const sumk_tf_layer_grads* layer_grads, float* dnorm_w, float* dnorm_b, float* dx, void* workspace,
                             size_t workspace_bytes, void* stream);
typedef struct sumk_tf_dec_layer_weights {
  const float* sa_in_w; const float* sa_in_b; const float* sa_out_w; const float* sa_out_b;   /* self_attn      (3D,D),(3D),(D,D),(D) */
  const float* ca_in_w; const float* ca_in_b; const float* ca_out_w; const float* ca_out_b;   /* multihead_attn (3D,D),(3D),(D,D),(D) */
  const float* lin1_w; const float* lin1_b; const float* lin2_w; const float* lin2_b;         /* (F,D),(F),(D,F),(D)                  */
  const float* norm1_w; const float* norm1_b; const float* norm2_w; const float* norm2_b;
  const float* norm3_w; const float* norm3_b;                                                 /* (D)                                  */
} sumk_tf_dec_layer_weights;
typedef struct sumk_tf_dec_layer_grads {   /* same fields, same shapes */
  float* sa_in_w; float* sa_in_b; float* sa_out_w; float* sa_out_b; float* ca_in_w; float* ca_in_b; float* ca_out_w; float* ca_out_b;
  float* lin1_w; float* lin1_b; float* lin2_w; float* lin2_b; float* norm1_w; float* norm1_b; float* norm2_w; float* norm2_b;
  float* norm3_w; float* norm3_b;
} sumk_tf_dec_layer_grads;
size_t sumk_tf_decoder_workspace_bytes(int32_t D, int32_t F, int32_t n_heads, int32_t n_layers, int32_t n_seq,
                                       const int32_t* seq_off_host);
/* tgt, memory (n_rows,D), packed with the SAME segment table (video v attends over its own memory rows) -> out (n_rows,D):
 * per layer norm1(t + SA(t)), norm2(. + CA(., memory)), norm3(. + FF(.)).  The memory's K / V projections of every layer are
 * computed up front.  training != 0 allows dropout. */
int sumk_tf_decoder_forward(const float* tgt, const float* memory, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                            int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                            const sumk_tf_dec_layer_weights* layers, const sumk_tf_opts* opts, float* out, void* workspace,
                            size_t workspace_bytes, int32_t training, void* stream);
/* Backward of sum(dout * out) after sumk_tf_decoder_forward on the same workspace: dtgt and dmemory (each if non-NULL) are
 * WRITTEN, dmemory summed over every layer's cross-attention. */
int sumk_tf_decoder_backward(const float* tgt, const float* memory, int32_t D, int32_t F, int32_t n_heads, int32_t n_layers,
                             int32_t n_seq, const int32_t* seq_off_host, const int32_t* seq_off_dev,
                             const sumk_tf_dec_layer_weights* layers, const sumk_tf_opts* opts, const float* dout,
                             const sumk_tf_dec_layer_grads* layer_grads, float* dtgt, float* dmemory, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Row scaling y[r,:] = x[r,:] * s[r] (sumgan_att.py:117) and its backward: dx[r,:] = s[r] g[r,:] (written if dx non-NULL),
 * ds[r] = <x[r,:], g[r,:]> (written if ds non-NULL).  D % 4 == 0. */
int sumk_row_scale_forward(const float* x, const float* s, int64_t n_rows, int32_t D, float* y, void* stream);
int sumk_row_scale_backward(const float* x, const float* s, const float* g, int64_t n_rows, int32_t D, float* dx, float* ds,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUMK_H */
