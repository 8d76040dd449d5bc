// Internal interface of the Transformer layer code (transformer.hip) shared with the encoder-stack and decoder-stack entries
// (tf_decoder.hip): the scorer's path plan, workspace carve-up, per-(video, head) problem tables, and the exact-fp32 blocks of a
// post-norm layer -- projections, the attention core (dense over a (video, head) table, or the stream form), the ReLU feed-forward --
// forward and backward.
#pragma once
#include "sumk_internal.h"

namespace sumk {

struct TfSeq { int64_t eoff; int32_t row0, T, ldE, pad_; };   // eoff: offset of this video's [heads][T][ldE] logits block

struct TfWs {
  size_t qkv, e, ctx, h0, h1, h2, t1, ff, seq, prob_row, prob_tabs, total;
  // training: per-layer saves (offset of layer 0 + l * lay_stride) and backward scratch
  size_t lay0, lay_stride, l_qkv, l_p, l_pd, l_ctx, l_t1a, l_hmid, l_ff, l_t1b, l_hout, l_stats;
  size_t hfin, z, stats_fin, scores, g0, g1, g2, dqkv, dff, lnpart, colpart, slab, prob_sk;
  size_t slab_elems;
  int64_t e_elems; int32_t n_rows;
  size_t as_seq;   // the stream carves: attn_stream.hip's descriptors (training: with attn_stream_bwd.hip's delta behind them); they
                   // have no `e`, `seq`, `prob_tabs`, `l_p`, `l_pd`
  size_t l_astats; // the stream training carve: per layer, the attention statistic (m, l) per (row, head)
};
// per-(video, head) sub-problem tables, each n_seq * heads entries: logits, context, and the four attention-backward products
enum { TT_S = 0, TT_PV = 1, TT_DV = 2, TT_DP = 3, TT_DQ = 4, TT_DK = 5, TT_COUNT = 6 };
constexpr int TF_SPLITK_PROBS = 64, TF_COLSUM_CHUNKS = 128;

struct TfGeom { TfWs L; int R, dh, tiles_s, tiles_pv, c_qkv, c_dd, c_df; };
// single-problem tables at TfWs::prob_row
enum { P_QKV = 0, P_DD = 1, P_DF = 2, P_FD = 3, P_DQKV = 4, P_NN_DF = 5, P_NN_FD = 6 };

int tf_carve(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, int training, TfWs* w);
int tf_geometry(int D, int F, int heads, int n_layers, int n_seq, const int32_t* off, int training, TfGeom* G);
// head_tables = false: only the single-problem tables (the stream path has no per-(video, head) GEMMs)
int tf_tables(const TfGeom& G, int D, int F, int heads, int n_seq, const int32_t* off_dev, char* ws, hipStream_t stream,
              bool head_tables = true);

__global__ void tf_softmax_kernel(float* E, float* E2, const TfSeq* seq, const int32_t* off, int n_seq, int n_rows, int heads,
                                  float scale, Drop drop, uint32_t site);
__global__ void tf_softmax_bwd_kernel(const float* E, float* E2, const TfSeq* seq, const int32_t* off, int n_seq, int n_rows,
                                      int heads, float scale, Drop drop, uint32_t site);
__global__ void mask_scale_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n, Drop drop, uint32_t site);

// The plane path of the dense scorer (inference in bf16x6 / bf16x3 with the weights' planes given): two activation-plane buffers behind
// the carve and, when the batch is eligible (`attn`: T <= 320, heads of 128 columns -- attn_pw.hip's multi-head form), the attention on
// planes too: [Q | K | V] planes written by the in-projection's epilogue, one set of alpha planes per head, the SeqInfo table.
struct TfPwExtra { size_t pa, pb, qp, ap, seqinfo, total; bool attn; int t_max; };

// The scorer's one plan: which attention, in which mode and arithmetic, and where everything lies in the workspace.  tf_plan is the only
// place that checks a call's shapes and sizes it; every size query, the forward and the backward of transformer.hip read it and nothing else.
enum { TF_DENSE = 0, TF_STREAM = 1, TF_STREAM_SPLIT = 2 };   // TF_STREAM_SPLIT: the stream form with the attention in `attn_prec`
struct TfPlan {
  bool stream;       // attention core: false the dense one (logits per (video, head)), true attn_stream*.hip (no logits in the carve)
  int training;      // the carve keeps every layer's activations for the backward
  int attn_prec;     // stream: 0 exact fp32 (attn_stream.hip / attn_stream_bwd.hip), SUMK_PRECISION_BF16X3 the *_split units
  int planes;        // dense scoring with the weights' planes given: their count (3: bf16x6, 2: bf16x3) -- the plane path; else 0
  TfGeom G;          // geometry and carve
  TfPwExtra px;      // planes != 0: the plane buffers behind the carve
  size_t tail, tail_bytes;   // what lies behind the carve (at tail = G.L.total): the bf16x3 attention's descriptors, (training: delta) and
                             // planes of ONE layer, or the plane path's buffers
  size_t total;
};
// what: the entry's name for the messages.  opts = null: a size query (nothing about the call's options is checked; a dense query that
// wants the plane path passes opts with `precision` and a non-null `wplanes`).
int tf_plan(const char* what, int attn, int training, int attn_prec, int D, int F, int heads, int n_layers, int n_seq, const int32_t* off_host,
            const sumk_tf_opts* opts, TfPlan* P);

// One call's geometry and workspace as the blocks below see it
struct TfRun {
  const TfGeom* G; char* ws; int D, F, heads, n_seq; const int32_t* off_dev; int precision; hipStream_t stream;
  const int32_t* off_host;   // the stream form of the attention blocks needs the host offsets too (null elsewhere)
  const TfPlan* plan;        // the scorer's plan (null in the stack entries of tf_decoder.hip: dense attention)
};
struct TfAttnW { const float* in_w; const float* in_b; const float* out_w; const float* out_b; };
struct TfAttnG { float* in_w; float* in_b; float* out_w; float* out_b; };
struct TfFfW { const float* w1; const float* b1; const float* w2; const float* b2; };
struct TfFfG { float* w1; float* b1; float* w2; float* b2; };

// [Q|K|V] (R,3D) = hin Win^T + bin
int tf_in_proj(const TfRun& r, const float* hin, const float* in_w, const float* in_b, float* QKV);
// T (R,D) = dropout(CTX Wo^T + bo, site) + hres
int tf_out_proj(const TfRun& r, const float* CTX, const float* out_w, const float* out_b, const float* hres, float* T, Drop dl,
                uint32_t site);
// attention core over one (video, head) table set `tabs` (TT_COUNT * n_seq * heads entries): E = Q K^T per sub-problem, softmax
// (+ dropout of the weights at `site` into E2 when dl is on), CTX = alpha V.  Q is addressed from `qbase`, K and V from `kvbase`.
int tf_attn_core_fwd(const TfRun& r, const GemmProb* tabs, const float* qbase, const float* kvbase, float* E, float* E2, float* CTX,
                     Drop dl, uint32_t site);
// its backward given dCTX: dV, dAlpha (into E2), softmax backward (in place on E2), dQ, dK.  dQ / dK / dV land where the table's
// TT_DQ / TT_DK / TT_DV entries point from `dq_base` / `dkv_base`.
int tf_attn_core_bwd(const TfRun& r, const GemmProb* tabs, const float* qbase, const float* kvbase, const float* P, float* E2,
                     const float* dCTX, float* dq_base, float* dkv_base, Drop dl, uint32_t site);
// the stream form of the two cores above for self-attention on the in-place [Q | K | V] (R,3D) buffer; needs r.plan (its attn_prec picks the
// unit, its tail holds the bf16x3 workspace).  astats (R, heads, 2): the statistic the training forward saves for the backward; null: the
// scoring launches, which keep none.
int tf_attn_stream_fwd(const TfRun& r, const float* QKV, float* CTX, float* astats, Drop dl, uint32_t site);
int tf_attn_stream_bwd(const TfRun& r, const float* QKV, const float* CTX, const float* dCTX, const float* astats, float* dQKV, Drop dl,
                       uint32_t site);
// self-attention block without its norm: T1a = dropout1(SA(hin)) + hin   (sites site+0: weights, site+1: dropout1)
// r.plan->stream: the stream form of the core (E, E2 unused; astats as tf_attn_stream_fwd)
int tf_sa_fwd(const TfRun& r, const TfAttnW& W, const float* hin, float* QKV, float* E, float* E2, float* CTX, float* T1a, Drop dl,
              uint32_t site, float* astats = nullptr);
// backward of tf_sa_fwd: dT (in: dT1a, out: dHin = dT1a + the attention path); s1, s2 (R,D) scratch; dQKV (R,3D) scratch
// astats non-null: the stream form of the core (P, E2 unused)
int tf_sa_bwd(const TfRun& r, const TfAttnW& W, const TfAttnG& Gd, const float* hin, const float* QKV, const float* P, float* E2,
              const float* CTX, float* dT, float* s1, float* s2, float* dQKV, Drop dl, uint32_t site, const float* astats = nullptr);
// feed-forward block without its norm: T = dropout_b(lin2(dropout_a(relu(lin1(h))))) + h   (sites site_a, site_b)
int tf_ff_fwd(const TfRun& r, const TfFfW& W, const float* h, float* FF, float* T, Drop dl, uint32_t site_a, uint32_t site_b);
// backward of tf_ff_fwd: dT (in: dT, out: dH = dT + the feed-forward path); s1 (R,D) scratch; dFF (R,F) scratch
int tf_ff_bwd(const TfRun& r, const TfFfW& W, const TfFfG& Gd, const float* h, const float* FFa, float* dT, float* s1, float* dFF,
              Drop dl, uint32_t site_a, uint32_t site_b);
// out[M,N] += dY^T Xin over the R rows (deterministic split-K)
int tf_wgrad(const TfRun& r, const float* dY, int ldy, int M, const float* Xin, int ldx, int N, float* out);
// C (R,N) (op)= A (R,K) . B (K,N) on the single-problem table `prob`
int tf_nn(const TfRun& r, const float* A, const float* B, float* C, int prob, GemmEpi epi, int N);

}  // namespace sumk
