/* openeat_hip.h - C ABI of libopeneat_hip.so (gfx950 / MI355X).
 *
 * The reference (TongtongSong/OpenEAT) owns no native code: its hot path is
 * Python nn.Modules whose arithmetic is done by aten kernels.  This library
 * is what replaces those aten calls.  Every entry point below names the
 * reference call site (file:line under /root/reference) whose device work it
 * performs; the Python mirror of the reference's module API
 * (openeat_amd/{models,modules,utils}) binds them through ctypes - see
 * INTEGRATION.md for the reference-side binding.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, scalars; no framework types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - tensors are dense row-major fp32 unless stated; lengths/labels int32.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is enqueued asynchronously on it; no call synchronises or allocates.
 *   - return 0 on success, non-zero on error (-1: invalid argument; >0: a
 *     hipError_t); oe_last_error() returns a thread-local message.
 *   - activations: 0 none, 1 relu, 2 swish (x*sigmoid(x)).
 */
#ifndef OPENEAT_HIP_H
#define OPENEAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* oe_last_error(void);
int oe_abi_version(void);

/* Capture hygiene (host only): while `origin` is capturing, how many of the `n_sides` streams hold captured work of the same
 * capture that the origin's next launch would NOT be ordered after (forks that have not been led back).  Returns that
 * count (0 = every fork rejoined; *unjoined_index = first offender), or -1 on error.  No reference counterpart: the
 * reference's step is not captured. */
int oe_capture_unjoined_streams(void* origin, void* const* sides, int n_sides, int* unjoined_index);

/* Diagnostic: when `stream` reaches this point, write the device's constant-rate wall clock (100 MHz ticks) into
 * buf[slot] (device memory).  Captured into a graph it times the replay's phases without a profiler. */
int oe_stamp(long long* buf, int slot, void* stream);

/* ------------------------------------------------------------------------- *
 * GEMM with fused epilogue.  C[m,n] = epi( alpha * sum_k A(m,k) B(n,k) )
 * Replaces aten::addmm/mm/bmm behind every torch.nn.Linear and 1x1 Conv1d of
 * the path: positionwise_feed_forward.py:43, attention.py:56-58,97,185,
 * subsampling.py:113, convolution.py:103,113, ctc.py:38, decoder.py:192, and
 * their backward (executor.py:56).  With conv_gather it is the implicit GEMM
 * of Conv2d(d,d,3,2) (subsampling.py:79) over an NHWC activation.
 *   a_kmajor/b_kmajor: 0 = operand stored [rows][k] (k contiguous),
 *                      1 = operand stored [k][rows].
 *   epilogue order: v = alpha*acc (+bias[n]) ; preact_out <- v ;
 *     v = actgrad_in ? v*act'(actgrad_in[m,n]) : act(v) ; dropout(drop_p,seed,
 *     index m*n_cols+n) ; rowmask[m]==0 -> 0 ; v = beta*v (+ residual[m',n],
 *     m' = m % res_row_mod when res_row_mod > 0: a (T,d) table broadcast over
 *     the batch, i.e. x*sqrt(d)+pe of embedding.py:59) ;
 *     C = v | C += v (accumulate) | atomicAdd (atomic_out, required when
 *     split_k > 1; C must hold the running value, e.g. zeros).
 *   beta must be set (1.0 = plain).  Dropout masks are a pure function of
 *   (seed + *seed_dev * golden, element index): the same arguments regenerate
 *   the mask in backward; seed_dev (optional device counter) lets a captured
 *   HIP graph draw fresh masks on every replay.
 * ------------------------------------------------------------------------- */
enum { OE_GATHER_NONE = 0, OE_GATHER_A = 1, OE_GATHER_B = 2 };

typedef struct oe_gemm_args {
    const float* a; long lda; int a_kmajor;
    const float* b; long ldb; int b_kmajor;
    float* c; long ldc;
    int m, n, k;
    int split_k;
    float alpha; const float* alpha_dev;
    const float* bias;
    int act;
    float* preact_out; const float* actgrad_in; long ld_aux;
    float drop_p; unsigned long long seed; const unsigned long long* seed_dev;
    const unsigned char* rowmask;
    const float* residual; long ldr; int res_row_mod; float beta;
    int accumulate; int atomic_out;
    int conv_gather; int conv_t1, conv_f1, conv_t2, conv_f2, conv_c;   /* implicit conv: input (B,t1,f1,c) NHWC -> (B,t2,f2) positions */
    float* a_colsum; /* optional (precision != 0, k-major A): a_colsum[m] += alpha * sum_k A(m,k), i.e. the bias
                        gradient fused into the weight-gradient GEMM (adders per address = split_k) */
    int precision;   /* 0: fp32-input MFMA (exact fp32 products); 1: bf16 inputs, fp32 accumulate;
                        3: 3-term bf16 split hi*hi+hi*lo+lo*hi (~2^-17 relative error per product);
                        6: 6-term bf16 split - three exact bf16 pieces per operand, h+m+l = x, products
                           hh+hm+mh+mm+hl+lh: what is dropped is < 2^-24 |a||b|, one fp32 rounding - the mode
                           that stands in for the reference's fp32 Linear / Conv products */
    int conv_k, conv_s;   /* kernel size / stride of the gathered conv; 0 = 3 / 2 (Conv2dSubsampling4/8); 5 / 3 is
                             Conv2dSubsampling6's second conv (subsampling.py:136) */
    int conv_kh;          /* kernel HEIGHT when it differs from conv_k (= width); 0 = square.  The gathered window may be
                             smaller than the input allows (conv_t2 <= (conv_t1 - kh) / s + 1): a sub-grid of positions */
    /* Output row scatter (0 = off): logical row r = (b, t, f) over (sc_t2, sc_f2) is stored at row
     * (b*sc_t1 + sc_s*t)*sc_f1 + sc_s*f of C (row stride ldc) and reads its actgrad_in row there too.  With conv_gather
     * on a zero-padded dy this makes the transposed (stride-2) convolution an implicit GEMM per output-parity class that
     * writes the input gradient in place (no column buffer): the (parity) base offsets go into the c / actgrad_in
     * pointers.  Not with atomic_out / accumulate / preact_out / residual / rowmask / dropout. */
    int out_scatter; int sc_t1, sc_f1, sc_t2, sc_f2, sc_s;
    /* Pre-split operands (precision 6 only; all optional, null = absent).  a_planes / b_planes: plane 0 of a copy of A / B
     * as three bf16 planes p0 + p1 + p2 = x (oe_split_planes, or a producer's planes output), same logical layout and
     * leading dimensions as a / b, plane n at + n * plane_stride ELEMENTS; when both are given and the problem qualifies
     * (16-byte alignment, leading dimensions and K multiples of 8 / the K-tile) the product runs on gemm_pl.hip - tiles
     * by LDS-DMA, no conversion in the loop.  b_planes ALONE (a_planes NULL; a row-major A, no gather, no split of the reduction):
     * the weight operand of a Linear taken from its pre-split copy, the activation split on the fragment (gemm_hyb.hip) - half the
     * conversion work of the all-fp32 kernels for nothing but the weights' one split per optimizer step.  c_planes: ALSO write the
     * output as planes (row stride ldcp): the next GEMM's operand without a pass over it. */
    const void* a_planes; long a_plane_stride;
    const void* b_planes; long b_plane_stride;
    void* c_planes; long c_plane_stride; long ldcp;
    /* conv_gather == OE_GATHER_A on pre-split operands only: order of the reduction index.  0 = (kh, kw, ci) as everywhere
     * else; 1 = channel-chunk major, k = ((ci / 32) * KH * KW + kh * KW + kw) * 32 + ci % 32 (C % 32 == 0; the caller lays B's
     * columns out in the same order): the K-loop then visits the KH * KW taps of one 32-channel chunk back to back, so the
     * overlapping windows of neighbouring output positions are re-read from L2 instead of HBM (conv2 forward at config 2:
     * 2.2 GB -> 1.0 GB fetched).  The launch fails if the pre-split kernel does not take the problem. */
    int conv_korder;
    /* actgrad_in points at bf16 values (ld_aux counts elements) instead of fp32 - with act = relu only, where nothing but the
     * sign of the source is read: plane 0 of an activation that exists as bf16 planes alone (the conv1 output of the
     * subsampling front end, whose fp32 copy - 636 MB at config 2 - is then never written or read). */
    int actgrad_bf16;
    /* Weight gradients (a_kmajor && b_kmajor, atomic_out) on pre-split operands whose reduction length k is NOT a multiple of 16
     * (ragged batches: k = valid rows of the step): set when BOTH planes buffers hold at least ceil(k / 16) * 16 rows and A's rows
     * beyond k are ZERO (openeat_amd.planes.alloc pads every buffer that way); a gathered B is read at clamped positions there.
     * The pre-split kernel then runs the padded length; without the flag such a k leaves it to the kernels that split in the loop
     * (configs[4], 24L d = 512: the conv2 weight gradient over k = 222 547 positions took 57.9 ms there, a third of the step). */
    int planes_k_padded;
} oe_gemm_args;

int oe_gemm_f32(const oe_gemm_args* args, void* stream);

/* x (rows, cols) fp32, row stride ld -> three bf16 planes p0 + p1 + p2 = x EXACTLY (round-to-nearest pieces of 8 significant
 * bits each), plane n at planes + n * plane_stride elements, row stride ldp: the pre-split operand format of oe_gemm_f32
 * precision 6 (a_planes / b_planes).  cols % 8 == 0, 16-byte aligned pointers.  Replaces the in-kernel splitting of
 * every consumer by one pass (Linear operands: positionwise_feed_forward.py:36-43, attention.py:36-63). */
int oe_split_planes(const float* x, long ld, long rows, long cols, void* planes, long ldp, long plane_stride, void* stream);
/* how many oe_gemm_f32 calls of this process ran on the pre-split kernel (gemm_pl.hip) so far: tests and tools check that a
 * problem they meant for it did not silently take the splitting kernels */
long oe_gemm_pl_launches(void);
/* launches of the weight-operand-only kernel (gemm_hyb.hip: b_planes alone) so far - tests assert a problem meant for it took it */
long oe_gemm_hyb_launches(void);
/* dispatch knobs of the pre-split kernel, for tests and tuning tools (-1 keeps a value): the smallest grid it accepts
 * (default 96 blocks: below that the splitting kernels' smaller tiles / split-K fill the chip better), a forced tile (22 =
 * 128 x 128, 11 = 64 x 64, 0 = automatic), a forced K-tile (16 / 32, 0 = automatic), waves per 128 x 128 block (8 / 4) */
int oe_gemm_pl_config(int min_blocks, int tile, int bk, int waves);
/* 1 (default, OE_PL_HYBRID): a row-major x row-major problem that runs on 128 x 256 tiles takes whole rounds of the chip on 256 x 256
 * tiles first (rows [0, m1)) and the rest on 128 x 256 (two launches, same operands) where that is fewer tile-rounds: the conv2 forward
 * and input-gradient GEMMs of subsampling.py:88-93.  -1 only reads.  Returns the previous setting. */
int oe_gemm_pl_hybrid(int on);

/* ------------------------------------------------------------------------- *
 * Position-wise feed forward as one kernel (positionwise_feed_forward.py:36-43 with the caller's residual / dropout of
 * encoder_layer.py:81-83,104-106, decoder_layer.py:104-106):
 *     y = residual + beta * drop_out( W2 . drop_in( act( W1 x + b1 ) ) + b2 )
 * on the bf16 matrix cores (precision 1 or 3, as oe_gemm_args.precision); the (rows, ff) intermediate stays in
 * registers.  The weights are consumed pre-split and in MFMA-fragment order: oe_ffn_pack_weights writes W1 (ff, d) and
 * W2 (d, ff) into w1p / w2p (oe_ffn_packed_bytes each) and must be re-run whenever the weights change.
 * oe_ffn_supported: d in {128, 256}, ff a multiple of 128, act 0 / 1 / 2 (none, relu, swish), precision 1 / 3 - anything
 * else is the caller's two oe_gemm_f32 launches.  pre_out / act_out (optional, (rows, ff) dense): the pre-activation
 * W1 x + b1 and the dropped activation, for the backward GEMMs; act_out needs pre_out.  Dropout masks are those of
 * oe_gemm_f32's epilogue on the same tensors (element index row * ff + col with seed_in, row * d + col with seed_out,
 * seed_dev mixed in the same way), so oe_gemm_f32 / oe_dropout_scale regenerate them in backward.
 * All pointers 16-byte aligned, ldx / ldr / ldy multiples of 4.
 * ------------------------------------------------------------------------- */
/* LayerNorm-backward PROLOGUE of a row-block kernel (oe_rowgemm6 at k = 256, oe_ffn_bwd at d = 256, precision 6): when dy != NULL the
 * kernel's input rows are not read but MADE, as
 *     dx = add + LN'(dy; x, stats (mean, rstd per row), gamma),   g = g_alpha * dropmask(g_p, g_seed, seed_dev) * g_rowmask * dx
 * i.e. oe_layernorm_bwd_dx_drop's two outputs (written to dx / g, both (rows, 256) contiguous), g feeding the kernel's product; ws
 * receives the parameter-gradient partials in oe_layernorm_bwd_workspace_floats' layout for oe_layernorm_param_reduce(_table).
 * (encoder_layer.py:79-106: the backward of every `x = residual + dropout(f(norm(x)))` starts from this g, and the LayerNorm
 * backward that makes it used to be a launch of its own.)  ln_rowmask: the LayerNorm's own row mask (rows with 0: dx = add, no
 * parameter gradient) or NULL.  The seed_dev of the enclosing argument block is the one mixed into g_seed. */
typedef struct oe_ln_prologue {
    const float* dy; const float* x; const float* stats; const float* gamma; const float* add;
    float* dx; float* g; float* ws;
    float g_alpha, g_p; unsigned long long g_seed; const unsigned char* g_rowmask; const unsigned char* ln_rowmask;
    /* PAIR (gamma2 != NULL): two norms back to back, y2 = LN2(u), u = LN1(x) (oe_layernorm_pair_bwd_dx_drop: encoder_layer.py:109-110
     * followed by the next layer's :79-80) - dy is then the gradient of y2, add the gradient that reaches u on its other path, x /
     * stats / gamma / beta belong to LN1 (u is recomputed), gamma2 / stats2 to LN2, ws2 receives LN2's parameter partials; no row mask. */
    const float* beta; const float* gamma2; const float* stats2; float* ws2;
} oe_ln_prologue;

/* LayerNorm-FORWARD prologue of a row-block kernel (oe_rowgemm6 at k = 256, oe_ffn_fwd at d = 256, precision 6): when x != NULL the
 * kernel's input rows are MADE as y = LayerNorm(x; gamma, beta, eps) (rows with rowmask 0: y = 0), written to y with the (mean, rstd)
 * pairs to stats - oe_layernorm_fwd's outputs - and fed to the product: the pre-norm of a residual block (encoder_layer.py:79-80,
 * 86-87, 92-93, 103-104) without a launch of its own. */
typedef struct oe_lnf_prologue {
    const float* x; const float* gamma; const float* beta; float eps;
    float* y; float* stats; const unsigned char* rowmask;
    /* PAIR (oe_ffn_fwd only; gamma2 != NULL): y = LN2(u; gamma2, beta2, eps2) with u = LN1(x; gamma, beta, eps) - norm_final of an encoder
     * layer and the next layer's first pre-norm (oe_layernorm_pair_fwd); u (optional output, the feed-forward's residual) and stats2 are
     * written too; no row mask. */
    const float* gamma2; const float* beta2; float eps2; float* u; float* stats2;
} oe_lnf_prologue;

/* LayerNorm-backward EPILOGUE of oe_rowgemm6 (row-block form, 256 <- 256): dx != NULL sends the product's rows dz through the backward of
 * z = act(LayerNorm(x; gamma, beta)) (act in OE_ACT_NONE / RELU / SWISH) with the forward's statistics - the conv module's norm +
 * activation between the depthwise convolution and pointwise_conv2 (convolution.py:107-111), whose input gradient the launch computes:
 * dx (rows, 256) receives the gradient of x, ws the parameter-gradient partials (oe_layernorm_bwd_workspace_floats' layout); y is not
 * written and no other epilogue feature applies. */
typedef struct oe_ln_epilogue {
    const float* x; const float* stats; const float* gamma; const float* beta; int act;
    float* dx; float* ws;
} oe_ln_epilogue;

typedef struct oe_ffn_args {
    const float* x; long ldx;                  /* (rows, d) */
    const void* w1p; const float* b1;          /* packed W1, bias (ff) or NULL */
    const void* w2p; const float* b2;          /* packed W2, bias (d) or NULL */
    int rows, d, ff, act, precision;
    float drop_in; unsigned long long seed_in;
    float drop_out; unsigned long long seed_out;
    const unsigned long long* seed_dev;
    float* pre_out; float* act_out;
    const float* residual; long ldr; float beta;
    float* y; long ldy;
    oe_ln_prologue ln;                          /* oe_ffn_bwd only (precision 6, d = 256): ln.dy != NULL makes the rows of dY (x is then ignored) */
    oe_lnf_prologue lnf;                        /* oe_ffn_fwd only (precision 6, d = 256): lnf.x != NULL makes the rows of x (x is then ignored) */
} oe_ffn_args;
size_t oe_ffn_packed_bytes(int d, int ff, int precision);
int oe_ffn_supported(int d, int ff, int precision, int act);
int oe_ffn_pack_weights(const float* w1, const float* w2, int d, int ff, int precision, void* w1p, void* w2p, void* stream);
int oe_ffn_fwd(const oe_ffn_args* args, void* stream);
/* The feed-forward's input gradient on the same kernel skeleton (autograd of positionwise_feed_forward.py:43):
 *   dH = (dY W2) * dropout mask(drop_in, seed_in) * act'(pre),  dX = dH W1.
 * oe_ffn_pack_weights_bwd packs W2^T in W1's role and W1^T in W2's role (buffers of oe_ffn_packed_bytes each).
 * oe_ffn_bwd reads oe_ffn_args as: x = dY (rows, d) after the output dropout / scale, w1p / w2p = those two streams,
 * pre_out = the forward's pre-activation (rows, ff) - an INPUT here -, act_out = dH (rows, ff) OUTPUT (the weight
 * gradient of W1 consumes it), y = dX (rows, d); b1, b2, residual unset, drop_out 0, beta 1. */
int oe_ffn_pack_weights_bwd(const float* w1, const float* w2, int d, int ff, int precision, void* w2t_packed, void* w1t_packed, void* stream);
int oe_ffn_bwd(const oe_ffn_args* a, void* stream);
/* The weights of n feed-forwards packed in ONE launch, both orientations (the optimizer moves every weight every step: 48 pack
 * launches per step at config 2 otherwise).  table: device array of n entries of NINE 64-bit words { W1, W2, w1p, w2p, w2t_packed,
 * w1t_packed, d, ff, planes } (device pointers as integers; planes = 1 / 2 / 3 for the precision the entry's buffers were sized for,
 * oe_ffn_packed_bytes; a null destination pair skips that orientation, an all-zero entry is skipped); max_d / max_ff: the largest
 * entry's sizes (launch geometry); precision: validated against max_d / max_ff only.  The table lives in device memory, so a captured graph can hold the launch. */
int oe_ffn_pack_weights_table(const void* table, int n, int max_d, int max_ff, int precision, void* stream);
/* precision 6 (csrc/ffn6.hip; d in {128, 256, 512}, three planes, oe_ffn_packed_bytes = 6 bytes per weight): block shape of the
 * fused kernel - 0 = automatic (32-row blocks of eight waves in two staggered groups wherever ff is a multiple of 256),
 * 1 = 64 rows / four waves (d <= 256), 2 = 32 rows / four waves, 3 = two groups; -1 only reads.  Returns the mode in force.
 * Tuning / tests only: results are identical in every mode up to the order of the fp32 sums over the ff axis. */
int oe_ffn6_config(int mode);

/* One Linear with a short reduction as a ROW-BLOCK GEMM in precision 6 (csrc/ffn6.hip, the fused feed-forward's first half alone):
 *     y[rows, n] = residual + beta * rowmask * dropout( x[rows, k] @ Wg[n, k]^T + bias ),   k in {256, 512}, n a multiple of 128;
 *     also k in {768, 1024} with n in {128, 256} (K-phased kernel: the input gradient through the fused q / k / v projection)
 * (attention.py:56-58,97 linear_q / k / v / out, convolution.py:79-111 pointwise convs, and - with Wg = W^T - their input
 * gradients).  wp: Wg as packed A-operand fragments (oe_rowgemm6_pack_table: 6 bytes per weight, refreshed whenever the weights
 * change).  Dropout / rowmask / residual as oe_gemm_f32's epilogue (mask element index row * n + col, seed_dev mixed in the same way).
 * All pointers 16-byte aligned, ldx / ldr / ldy multiples of 4. */
typedef struct oe_rowgemm_args {
    const float* x; long ldx;
    const void* wp; const float* bias;          /* packed Wg; bias (n) or NULL */
    int rows, k, n;
    float drop_p; unsigned long long seed; const unsigned long long* seed_dev;
    const unsigned char* rowmask;               /* (rows) or NULL: rows with 0 are zeroed before the residual is added */
    const float* residual; long ldr; float beta;
    float* y; long ldy;
    /* tile form only (oe_rowgemm6_form = 2), oe_gemm_f32's activation epilogue: act = OE_ACT_NONE / RELU / SWISH applied after the bias
     * (preact_out, optional: the value before it, row stride ld_aux), or - actgrad_in set - the product times act'(actgrad_in[row, col]) */
    int act; float* preact_out; const float* actgrad_in; long ld_aux;
    oe_ln_prologue ln;                          /* row-block form at k = 256: ln.dy != NULL makes the input rows (x is then ignored) */
    oe_lnf_prologue lnf;                        /* ... or lnf.x != NULL: a LayerNorm forward makes them */
    oe_ln_epilogue lne;                         /* lne.dx != NULL: the product leaves through a LayerNorm backward */
} oe_rowgemm_args;
int oe_rowgemm6_supported(int k, int n);
/* Which kernel oe_rowgemm6 runs: 1 = the row-block form above (k in {256, 512}, n % 128 == 0: one 32-row block streams the whole packed
 * matrix - for thousands of rows), 2 = the TILE form for few rows (rows <= 2048, k in {256, 512, 768, 1024}, n % 32 == 0: one block per
 * 32 x 32 output tile, its eight waves split the reduction - the decoders' Linears, decoder_layer.py:82-106), 0 = neither. */
int oe_rowgemm6_form(int rows, int k, int n);
int oe_rowgemm6(const oe_rowgemm_args* args, void* stream);
/* table: device array of n entries of six 64-bit words { W (device pointer), packed destination, R, Cc, row stride of W,
 * transposed }: W (R, Cc) fp32 -> the fragments of Wg = W (transposed 0: an (R, Cc) operand, x W^T) or Wg = W^T (transposed 1: a
 * (Cc, R) operand, dy W); max_pieces = the largest entry's (Wg rows / 32) * (Wg cols / 16).  One launch for every Linear of the model. */
int oe_rowgemm6_pack_table(const void* table, int n, long max_pieces, void* stream);

/* Several weight gradients  C_i (+)= alpha_i * A_i^T B_i  (A_i (k_i, m_i), B_i (k_i, n_i), both k-major, fp32) in ONE launch
 * of the bf16-planes kernel, accumulated atomically into C_i (ops.flush_wgrads: the deferred weight gradients of a captured
 * step; autograd of torch.nn.Linear in the reference).  oe_gemm_tn_grouped_plan fills the launch geometry fields of a HOST
 * array and returns the total block count (-1: a problem does not qualify: 16-byte aligned operands, leading dimensions
 * that are whole float4s and cover the rounded-up row lengths); the caller copies the array to device memory and passes it
 * to oe_gemm_tn_grouped.  a_colsum (optional): alpha_i * column sums of A_i are added to it (fused bias gradient). */
typedef struct oe_tn_problem {
    const float* a; const float* b; float* c; float* a_colsum; const float* alpha_dev;
    long lda, ldb, ldc;
    int m, n, k;
    float alpha;
    int k_chunk, gx, gy, nz, block_start, reserved;      /* filled by oe_gemm_tn_grouped_plan */
} oe_tn_problem;
int oe_gemm_tn_grouped_plan(oe_tn_problem* problems_host, int n, int target_blocks);
int oe_gemm_tn_grouped(const oe_tn_problem* problems_dev, int n, int total_blocks, int precision, void* stream);

/* column sums: out[n] (+)= alpha * sum_m x[m,n]  - bias gradients of every
 * Linear (autograd of aten::addmm).  alpha_dev optional device scalar. */
int oe_colsum_f32(const float* x, long ldx, int m, int n, float alpha, const float* alpha_dev,
                  float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------- *
 * LayerNorm over the last dim (torch.nn.LayerNorm in encoder_layer.py:54-62,
 * encoder.py:204, convolution.py:61, decoder_layer.py:43-45, decoder.py:163).
 * rowmask (optional, [rows] bytes): rows with 0 produce an all-zero output
 * row - the masked_fill_ of convolution.py:88-89 fused into norm_conv.
 * stats (optional out): [rows][2] = (mean, rstd) kept for backward.
 * act: activation applied to the normalised output (convolution.py:110:
 * activation(norm(x))); backward then needs beta to rebuild the pre-activation.
 * ------------------------------------------------------------------------- */
/* as oe_layernorm_fwd, plus y_planes (optional): y also as three bf16 planes (rows, d), plane_stride elements apart */
int oe_layernorm_fwd_pl(const float* x, const float* gamma, const float* beta, float eps, int rows, int d,
                        const unsigned char* rowmask, int act, float* y, float* stats, void* y_planes, long plane_stride, void* stream);
int oe_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, int rows, int d,
                     const unsigned char* rowmask, int act, float* y, float* stats, void* stream);
/* dx = LN'(dy) (+ add, optional: the residual branch's gradient of the
 * pre-norm blocks, may alias dx); dgamma/dbeta ACCUMULATED atomically (caller
 * zeroes them; block partials in `workspace` are summed in a fixed order:
 * deterministic).  rowmask as in forward (masked rows: LN'(dy) = 0, no
 * dgamma/dbeta contribution). */
size_t oe_layernorm_bwd_workspace_floats(int rows, int d);
int oe_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* beta, int act,
                     const float* stats, int rows, int d, const unsigned char* rowmask, const float* add,
                     float* dx, float* dgamma, float* dbeta, float* workspace, void* stream);
/* Two LayerNorms back to back in one pass, y2 = LN2(LN1(x)): the norms at an encoder layer boundary
 * (/root/reference/openeat/modules/encoder_layer.py:109-110 `x = norm_final(x)` followed by the next layer's :79-80
 * `x = norm_ff_macaron(x)`, or encoder.py's after_norm behind the last layer).  y1 (LN1's output, the next block's residual) may be
 * NULL when nothing else reads it; stats1 / stats2 = (mean, rstd) per row of each norm.  The backward takes dy2 (gradient of
 * y2) and `add` (the gradient reaching y1 on its other path, NULL: none), recomputes y1 from x, and writes dx (plus the optional
 * dropped copy gout of oe_layernorm_bwd_dx_drop) and the partial parameter-gradient rows of LN1 / LN2 into workspace1 / workspace2
 * (oe_layernorm_bwd_workspace_floats(rows, d) floats each; summed by oe_layernorm_param_reduce[_table]). */
int oe_layernorm_pair_fwd(const float* x, const float* gamma1, const float* beta1, float eps1, const float* gamma2, const float* beta2,
                          float eps2, int rows, int d, float* y1, float* stats1, float* y2, float* stats2, void* stream);
int oe_layernorm_pair_bwd_dx_drop(const float* dy2, const float* x, const float* gamma1, const float* beta1, const float* stats1,
                                  const float* gamma2, const float* stats2, int rows, int d, const float* add, float* dx, float* gout,
                                  float g_alpha, float g_p, unsigned long long g_seed, const unsigned long long* g_seed_dev,
                                  const unsigned char* g_rowmask, float* workspace1, float* workspace2, void* stream);
/* The same split in two: oe_layernorm_bwd_dx writes dx and the per-block partial sums of the parameter gradients into
 * `workspace`; oe_layernorm_param_reduce_table reduces the partials of n such calls with ONE launch.  table (device
 * memory) holds 5 int64 words per call: { workspace pointer, rows, d, dgamma pointer, dbeta pointer } (a null workspace
 * pointer skips the entry); max_rows / max_d bound the entries' rows / d.  dgamma / dbeta are accumulated atomically.
 * Every workspace must stay untouched until the reduction has run.  (A captured graph can hold the launch while the
 * host fills the table after the capture: 93 reductions of 4.6 us each become one launch at config 2.) */
int oe_layernorm_bwd_dx(const float* dy, const float* x, const float* gamma, const float* beta, int act, const float* stats,
                        int rows, int d, const unsigned char* rowmask, const float* add, float* dx, float* workspace,
                        void* stream);
int oe_layernorm_param_reduce(const float* workspace, int rows, int d, float* dgamma, float* dbeta, void* stream);   /* one call's partials */
int oe_layernorm_param_reduce_table(const long long* table, int n, int max_rows, int max_d, void* stream);
/* oe_layernorm_bwd_dx with a second output gout = g_alpha * keep(g_seed, element)/(1 - g_p) * dx, rows with
 * g_rowmask[row] == 0 zeroed: oe_dropout_scale applied to dx (same mask definition, d % 8 == 0).  dx of a pre-norm
 * block's LayerNorm is the gradient of the PREVIOUS block's output `residual + out_scale * dropout(f(.))`
 * (encoder_layer.py:83,89,95,106), whose backward starts by applying exactly that mask and scale. */
int oe_layernorm_bwd_dx_drop(const float* dy, const float* x, const float* gamma, const float* beta, int act,
                             const float* stats, int rows, int d, const unsigned char* rowmask, const float* add, float* dx,
                             float* gout, float g_alpha, float g_p, unsigned long long g_seed,
                             const unsigned long long* g_seed_dev, const unsigned char* g_rowmask, float* workspace,
                             void* stream);
/* ... plus out_planes (optional): three bf16 planes (rows, d) of gout when gout is given, else of dx - the tensor the
 * previous block's GEMMs read as an operand (oe_gemm_args.a_planes) */
int oe_layernorm_bwd_dx_drop_pl(const float* dy, const float* x, const float* gamma, const float* beta, int act,
                                const float* stats, int rows, int d, const unsigned char* rowmask, const float* add, float* dx,
                                float* gout, float g_alpha, float g_p, unsigned long long g_seed,
                                const unsigned long long* g_seed_dev, const unsigned char* g_rowmask, float* workspace,
                                void* out_planes, long plane_stride, void* stream);

/* ------------------------------------------------------------------------- *
 * CTC head: log_softmax + CTCLoss(reduction='sum', zero_infinity=True) and
 * its gradient w.r.t. the logits in one pass structure
 * (ctc.py:38-45: ctc_lo -> log_softmax(2) -> ctc_loss -> / B;  backward via
 * executor.py:56).  blank = 0.
 *   logits  (B, T, ldv>=V) batch-major, row stride ldv
 *   hlens   (B) valid frames, targets (B, Lmax) int32 (entries >= tlen ignored)
 *   utt_weight (B) or NULL: per-utterance weight w_b (NULL = 1).  CTC(length_normalized_loss=True)
 *        (ctc.py:24-25: CTCLoss(reduction='mean')) is w_b = 1 / max(tlen_b, 1) and a further / B on the host.
 *   out: nll (B) unweighted, infeasible -> 0;  loss_sum[0] = sum_b w_b * nll_b,
 *        dlogits (B, T, ldv) = grad_scale * d loss_sum / d logits (may alias
 *        logits; padded frames / infeasible utterances exactly 0), or NULL.
 *        Columns >= V of dlogits (the row padding) are never written.
 *   workspace: float[ oe_ctc_workspace_floats(B,T,Lmax) ].
 *   Two paths, chosen by the launch's T alone (every utterance of a launch takes the same one):
 *     T <= 248: alpha / beta / ll in float32.  The error of an occupancy grows with the utterance's negative
 *        log-likelihood; against a float64 loss the gradient holds rtol 2e-3 / atol 2e-5 * grad_scale * w_b up to
 *        |nll| ~ 2000 nats (measured: 0.7 of that tolerance at T = 248, V = 3246, untrained posteriors).  The launch forms
 *        of oe_ctc_config apply here.
 *     T  > 248: alpha / beta / ll in float64 (the recursion of oe_ctc_nbest_score), rows, alpha/beta, labels one after the
 *        other whatever oe_ctc_config says.  The same tolerance holds with a margin of 10x or more up to T = 2000 and
 *        |nll| ~ 22000 nats (tests/test_ctc_long_gpu.py).  The workspace grows by the two float64 trellises.
 *     Both: nll rtol 1e-4 / atol 1e-3; loss-only calls, in-place gradients, utt_weight, zero_infinity and graph capture.
 * ------------------------------------------------------------------------- */
size_t oe_ctc_workspace_floats(int B, int T, int Lmax);
/* oe_ctc_loss_fused launch form, for tests and tuning tools (-1 / 0 keeps a value): pipe_mode 0 = rows, alpha/beta, labels one
 * after the other (default); 1 = for large batches the recursion runs in `chunks` time chunks on two internal streams under
 * the dense passes' traffic (ordinary stream events; capturable; measured SLOWER on MI355X: each cross-stream edge costs
 * more than the chain time it hides); 2 = pipelined whatever the size.  Other values behave as 0. */
int oe_ctc_config(int pipe_mode, int chunks);
int oe_ctc_loss_fused(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* targets,
                      int Lmax, const int* tlens, float grad_scale, const float* utt_weight, float* nll, float* loss_sum,
                      float* dlogits, float* workspace, void* stream);

/* CTC greedy search on device (asr_model.py:318-325 + common.py:187-196):
 * argmax over V per frame (lowest index wins ties, = topk(1)), frames >= hlen
 * become `eos`, repeats merged, blanks dropped.  out_tokens (B, T) int32,
 * padded with -1; out_lens (B). */
int oe_ctc_greedy(const float* logits, long ldv, int B, int T, int V, const int* hlens, int eos,
                  int* frame_best, int* out_tokens, int* out_lens, void* stream);

/* CTC forced alignment on device: the best path through the trellis the loss sums over (ctc.py:27-45: blank, y1, blank, ..
 * blank; blank = 0) - token times and confidences.  The reference has no aligner (WeNet, which it derives from, has one);
 * these are the semantics every layer refers to.  With Tb = hlens[b], y = targets[b, :tlens[b]] (L labels),
 * lp = log_softmax(logits[b, t, :V]) in natural log and ext[s] = (s odd ? y[s >> 1] : 0), s = 0 .. 2L:
 *   v[0,0] = lp[0,0], v[0,1] = lp[0,ext[1]], every other state of frame 0 is -inf;
 *   v[t,s] = lp[t,ext[s]] + max(v[t-1,s], v[t-1,s-1], v[t-1,s-2]), the third term only for odd s >= 3 with ext[s] != ext[s-2];
 *   the path ends in state 2L or 2L-1, whichever has the larger v[Tb-1, .].
 *   Ties: a predecessor replaces the best only if strictly greater, tried in the order stay (s), step (s-1), skip (s-2);
 *   at the end 2L is kept unless 2L-1 is strictly greater.
 *   out: frames (B, T) int32 = ext[state_t] for t < Tb, -1 for t >= Tb;  tok_start / tok_end (B, Lmax) int32 = first / last
 *        frame (inclusive) spent in state 2l+1, -1 for l >= L;  tok_logp (B, Lmax) = sum of lp[t, y[l]] over those frames,
 *        0 for l >= L;  score (B) = v[Tb-1, final].  tok_start, tok_end, tok_logp may each be NULL.
 *   Infeasible utterances (Tb == 0, or fewer frames than L + adjacent repeats - what the loss calls infeasible): score -inf,
 *        frames / tok_start / tok_end all -1, tok_logp 0.  An empty target with Tb > 0 is feasible: every frame blank.
 *   logits, hlens, targets, tlens as oe_ctc_loss_fused (read only);  Lmax <= 255;
 *   workspace: oe_ctc_align_workspace_bytes(B,T,Lmax) bytes, 16-byte aligned.
 * Two launches (the loss's row pass, then one wave per utterance: recursion and back-trace); no allocation, no
 * synchronisation, no host-side state: capturable. */
size_t oe_ctc_align_workspace_bytes(int B, int T, int Lmax);
int oe_ctc_align(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* targets, int Lmax,
                 const int* tlens, int* frames, int* tok_start, int* tok_end, float* tok_logp, float* score, void* workspace,
                 void* stream);

/* Long-form CTC segmentation on device (CTC segmentation, Kuerzinger et al. 2020): the best path of a WHOLE RECORDING through
 * the trellis of its transcript - the utterances' labels concatenated - with the audio outside the transcript (intro, outro,
 * music, noise) free.  With Tb = hlens[b], y = targets[b, :tlens[b]] (L labels), lp, ext[s], S = 2L+1, the legal moves (stay,
 * step, skip) and the tie rule exactly as oe_ctc_align above (a predecessor replaces the best only if strictly greater, tried
 * in the order stay, step, skip; the end state 2L is kept unless 2L-1 is strictly greater), two flags change the recursion:
 *   free_start: state 0 costs nothing: v[t,0] = 0 for every t, t = 0 included.  Every other state follows oe_ctc_align's
 *        recursion (v[0,1] = lp[0,ext[1]]; state 1 may be entered from state 0 at any frame).
 *   free_end: staying in state 2L costs nothing and entering it costs the blank:
 *        v[t,2L] = max(v[t-1,2L], v[t-1,2L-1] + lp[t,0]), the step only if strictly greater (v[0,2L] = -inf for L > 0).
 *        L == 0 with free_start: the state-0 rule applies.  L == 0 with free_end only: v[0,0] = lp[0,0], the rest is free.
 *   A frame of the returned path is FREE if (free_start and state_t == 0) or (free_end and t > 0 and state_t == state_{t-1} == 2L).
 *   With both flags 0 the path problem is exactly oe_ctc_align's.  Feasibility does not change under the flags: infeasible is
 *   Tb == 0 or fewer frames than L + adjacent repeats; the outputs are then -inf / -1 / 0 as in oe_ctc_align.
 *   out (device memory):
 *        frames (B, T) int32 = ext[state_t], -1 for t >= Tb;
 *        path_logp (B, T) float32 or NULL = lp[t, ext[state_t]] in natural log, 0 on free frames and for t >= Tb;
 *        tok_start / tok_end / tok_logp (B, Lmax), each or NULL, as oe_ctc_align defines them;
 *        score (B) FLOAT64 = the path's log-probability: the float64 sum, in frame order, of the path_logp values; -inf if infeasible.
 *   A property, not a defect: a free state costs 0 and every scored frame costs less than 0, so under free_start the path
 *   leaves state 0 as late as it can and the first label's span comes out as short as optimality allows - the behaviour of
 *   CTC segmentation as published.
 *   The recursion accumulates in float32: the returned path is optimal up to float32 rounding of v (its float64 score is within
 *   a relative 1e-4 of the float64 optimum in the tests), and it is always a legal path that collapses to y.
 *   Labels are expected in [1, V); one outside [0, V) is read as the nearest valid column, never out of bounds.
 *   Limits: 1 <= B, 1 <= T <= 2^20, 0 <= Lmax <= 8191, V > 1, ldv >= V.  Anything else, and any NULL required pointer
 *   (logits, hlens, tlens, frames, score, workspace; targets unless Lmax == 0), is reported through oe_last_error before
 *   any launch, with the outputs untouched.
 *   workspace: oe_ctc_segment_workspace_bytes(B,T,V,Lmax) bytes, 16-byte aligned (0 for shapes outside the limits): 2 bits of
 *        back-pointer per cell and 12 bytes per frame - never a float per cell, never a T x S table:
 *        <= B * (T * (Sp/2 + 4*V + 64) + 65536) with Sp = 2*Lmax+1 rounded up to a multiple of 128.
 * Two launches (row statistics; one workgroup per recording: recursion, back-trace, spans, score).  No workgroup waits for
 * another, no atomics; no allocation, no host read, no host-side state: capturable. */
typedef struct oe_ctc_segment_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens; const int* targets; int Lmax; const int* tlens;
    int free_start, free_end;
    int* frames; float* path_logp; int* tok_start; int* tok_end; float* tok_logp; double* score;
    void* workspace;
} oe_ctc_segment_args;
size_t oe_ctc_segment_workspace_bytes(int B, int T, int V, int Lmax);
int oe_ctc_segment(const oe_ctc_segment_args* args, void* stream);

/* Keyword search over CTC posteriors on device (keyword spotting / spoken-term detection): for every recording b and every
 * keyword k of a list, WHERE the keyword occurs and how confidently - every occurrence, not one placement.  The reference has
 * none; these are the semantics every layer refers to.  With Tb = hlens[b], lp[t,v] the natural-log posterior, keyword k's
 * labels y = y_1..y_L (L = klens[k], 1 <= L <= 32) and ext[s] as in oe_ctc_align (odd s: y[s >> 1], even s: blank 0), only
 * the states 1 .. 2L-1 exist: a keyword starts in its first label and ends in its last, no blank state before or after it -
 * at most 63 states, one per lane of a wave.  Each state carries a value v (float32) and the frame st at which its path
 * entered state 1:
 *   v[t,s] = lp[t,ext[s]] + the best of   stay  v[t-1,s]
 *                                        step  v[t-1,s-1]   (s >= 2)
 *                                        skip  v[t-1,s-2]   (odd s >= 3 with ext[s] != ext[s-2])
 *                                        fresh 0, with st = t   (s == 1 only)
 *   tried in that order; a candidate replaces the best only if strictly greater (oe_ctc_align's tie rule) and st travels with
 *   the winner.  At t = 0 only fresh exists.  A state with no predecessor is unreachable, and an unreachable state is never a
 *   candidate below, whatever finite stand-in for -inf the kernel uses (lp is expected finite).
 *   Candidate: at every frame t at which state 2L-1 is reachable, the span [st, t] with n = t - st + 1 frames and the score
 *   sc = v[t,2L-1]: the log-probability of the best path that spells the keyword and ends at t, its start free.
 *   Comparisons between candidates are exact, in float64 and without a division: a is better than b iff
 *   (double)a.sc * b.n > (double)b.sc * a.n (the mean log-probability per frame); a candidate passes the threshold iff
 *   (double)sc >= (double)thr[k] * n.
 *   Hits: per (b,k), t ascending, one pending hit.  A passing candidate whose st <= the pending hit's end overlaps it and
 *   replaces it iff it is better; one that does not overlap has the pending hit emitted and becomes the pending one; after
 *   the last frame the pending hit is emitted.  The emitted hits are in time order and disjoint.
 *   out (device memory):
 *        n_hits (B, K) int32 = the number of hits emitted; may exceed max_hits;
 *        hit_start / hit_end (B, K, max_hits) int32 = the spans of the first max_hits hits, -1 in unused slots;
 *        hit_score (B, K, max_hits) float32 = their sc, 0 in unused slots;
 *        best_start / best_end (B, K) int32, best_score (B, K) float32, each or NULL = the best candidate over all frames
 *        whatever the threshold, the earliest kept on ties; -1 / -1 / -inf if there never was a candidate.
 *   klens[k] == 0 or Tb == 0: no hits, no best.  Tb is hlens[b] held to [0, T], L is klens[k] held to [0, Lmax].
 *   Labels are expected in [1, V); one outside [0, V) is read as the nearest valid column, never out of bounds, as in
 *   oe_ctc_segment; ext[s] != ext[s-2] compares the labels as given (their indices in cols).
 *   A property, not a defect: a fresh start costs 0 and every scored frame costs at most 0, so a span is as tight as
 *   optimality allows: it starts with the last frame of the first label's run and a candidate ends where the last label is
 *   entered or held.  A keyword of one label has one-frame candidates.
 *   normalized = 0: logits are raw and lp = logits - c_t with c_t the row's log-sum-exp;  normalized = 1: the rows are used as
 *   given (callers that hold log-probabilities; values on a coarse binary grid make every float32 sum exact).
 *   The keyword list is one struct, host memory read during the call only, its four pointers device pointers (built by
 *   openeat_amd/utils/keyword.py): cols (U) the distinct tokens of all keywords, ascending; kw_col (K, Lmax) the index into
 *   cols of each label (held to [0, U)); klens (K); thr (K) the mean natural-log-probability per frame a hit must reach.
 *   Limits: 1 <= B, 1 <= T <= 2^20, 1 <= K <= 65535, 1 <= Lmax <= 32, 1 <= U < V, ldv >= V, max_hits >= 1.  Anything else,
 *   and any NULL required pointer (logits, hlens, kws and its four tables, n_hits, hit_start, hit_end, hit_score, workspace),
 *   is reported through oe_last_error before any launch, with the outputs untouched.
 *   workspace: oe_ctc_kws_workspace_bytes(B,T,U) = B*T*(U+1) floats, 16-byte aligned (0 for shapes outside the limits): per
 *   frame the blank and the U keyword columns as lp.  Keywords are independent, so a caller short of memory runs them in groups.
 * Two launches (one wave per frame: every logits row is read once, its log-sum-exp taken and its U+1 columns kept; one wave
 * per (b,k): recursion and scan, the start frame carried, not traced - no (B,K,T) table, no back-pointers).  No workgroup
 * waits for another, no atomics; no allocation, no host read, no host-side state: capturable. */
typedef struct oe_keyword_set {
    const int* cols;      /* (U) the distinct tokens of all keywords, ascending */
    int U;
    const int* kw_col;    /* (K,Lmax) index into cols of each label */
    const int* klens;     /* (K) */
    const float* thr;     /* (K) mean natural-log-probability per frame a hit must reach */
    int K, Lmax;
} oe_keyword_set;
typedef struct oe_ctc_kws_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_keyword_set* kws;
    int normalized, max_hits;
    int* n_hits; int* hit_start; int* hit_end; float* hit_score;
    int* best_start; int* best_end; float* best_score;
    void* workspace;
} oe_ctc_kws_args;
size_t oe_ctc_kws_workspace_bytes(int B, int T, int U);
int oe_ctc_kws(const oe_ctc_kws_args* args, void* stream);

/* Grammar-constrained CTC decoding on device: the best path of the CTC posteriors through an epsilon-free weighted token graph
 * (a command list, a digit loop, words with several spellings, a transcript with alternatives), the CTC topology - blank,
 * repeats - applied implicitly.  The reference has none (WeNet, which it derives from, ships it as TLG decoding); these are the
 * semantics every layer refers to.
 *   Graph: Q nodes, node 0 the start; A arcs, arc a with src[a], dst[a], a label label[a] in [1, V) (blank, 0, is never a
 *   label) and a weight w[a] (float32, natural log, any finite value); final[q] float32, -inf = not final.  The graph may be
 *   non-deterministic and may have self-loops, parallel arcs and unreachable nodes; there are no epsilon arcs.  Arcs are
 *   stored sorted by dst, stable, with in_ptr (Q+1): the arcs into q are in_ptr[q] .. in_ptr[q+1]-1, and arc ids are positions
 *   in this order.  As in oe_keyword_set, cols (U) holds the distinct labels ascending and col[a] the index of label[a] into
 *   cols; "same label" means same col.  A label outside [0, V) is read as the nearest valid column, never out of bounds, as
 *   in oe_ctc_segment and oe_ctc_kws (src, dst, col and in_ptr are likewise held to their ranges).
 *   States, per utterance: a node state n[q] - the path is at q and the last frame was blank, or no frame was consumed yet -
 *   and an arc state r[a] - the last frame emitted label[a] while traversing a.  Before frame 0, n[0] = 0 and every other
 *   state is unreachable.  With Tb = hlens[b] held to [0, T] and lp as in oe_ctc_kws (normalized 0 or 1), for t = 0 .. Tb-1:
 *     r_t[a] = lp[t,label[a]] + the best of   stay       r_{t-1}[a]
 *                                             from node  n_{t-1}[src[a]] + w[a]
 *                                             from arc   r_{t-1}[a'] + w[a], every a' with dst[a'] == src[a] and a label
 *                                                        different from label[a]
 *     n_t[q] = lp[t,0] + the best of          stay       n_{t-1}[q]
 *                                             arrive     r_{t-1}[a'], every a' with dst[a'] == q
 *   Ties (oe_ctc_align's rule, generalised): candidates are tried in the order stay, from node, then arcs by ascending id; a
 *   candidate replaces the best only if strictly greater.  An unreachable state is never a candidate.
 *   End: the winner is the best of n_{Tb-1}[q] + final[q] over q ascending, then r_{Tb-1}[a] + final[dst[a]] over a ascending,
 *   a later candidate only if strictly greater.  Tb == 0 or no final state reachable: the utterance is infeasible.
 *   On a linear chain with zero weights this is exactly oe_ctc_align's problem, ties included.
 *   The recursion accumulates in float32 and adds w[a] to the maximum over the node and the arcs, not to each candidate: the
 *   same winner wherever the sums are exact (values on a coarse binary grid); elsewhere the path is optimal up to float32
 *   rounding and always a path the graph accepts.
 *   out (device memory):
 *        score (B) float32 = the winner's value, weights and final weight included; -inf if infeasible;
 *        frames (B, T) int32 = the label emitted at each frame (label[a] as given), 0 for blank, -1 for t >= Tb or infeasible;
 *        arcs (B, T) int32 = the arc id where the path is in an arc state, -1 elsewhere;
 *        path_logp (B, T) float32 or NULL = lp[t, frames[t]], 0 for t >= Tb or infeasible;
 *        n_trav (B) int32 = the number of arc traversals (0 if infeasible): a traversal starts at t iff arcs[t] >= 0 and
 *        (t == 0 or arcs[t-1] != arcs[t]); may exceed max_trav;
 *        trav_arc / trav_start / trav_end (B, max_trav) int32 = the first max_trav traversals, last frame inclusive, -1 in
 *        unused slots;  trav_logp (B, max_trav) float32 or NULL = the float32 sum, in frame order, of lp over the traversal's
 *        frames, 0 in unused slots.
 *   The graph is one struct, host memory read during the call only, its pointers device pointers (built by
 *   openeat_amd/utils/decoding_graph.py).
 *   Limits: 1 <= B, 1 <= T <= 2^20, V > 1, ldv >= V, 1 <= U < V, max_trav >= 1, 1 <= Q <= OE_CTC_GRAPH_MAX_NODES,
 *   1 <= A <= OE_CTC_GRAPH_MAX_ARCS: one workgroup holds 4 bytes per arc and 12 per node in the 160 KiB of LDS
 *   (4 * 16384 + 12 * 8064 = 158.5 KiB, the rest its lists and reduction slots).  Anything else, and any NULL required pointer
 *   (logits, hlens, graph and its eight tables, score, frames, arcs, n_trav, trav_arc, trav_start, trav_end, workspace), is
 *   reported through oe_last_error before any launch, with the outputs untouched.
 *   workspace: oe_ctc_graph_workspace_bytes(B,T,U,Q,A) bytes, 16-byte aligned (0 for shapes outside the limits):
 *   B*T*(U+1) floats of lp as in oe_ctc_kws, then per frame a 4-byte back-pointer word per node and a byte per arc:
 *   4 * B * T * (U + 1 + Q + ceil(A / 4)).  Utterances are independent, so a caller short of memory runs them in groups.
 * Two launches (the row pass of oe_ctc_kws; one workgroup per utterance: recursion with the state values in LDS, back-trace,
 * traversal list, score).  No workgroup waits for another, no float atomics; no allocation, no host read, no host-side state:
 * capturable. */
#define OE_CTC_GRAPH_MAX_NODES 8064
#define OE_CTC_GRAPH_MAX_ARCS 16384
typedef struct oe_decoding_graph {
    int Q, A;
    const int* in_ptr;    /* (Q+1) the arcs into q are in_ptr[q] .. in_ptr[q+1]-1 */
    const int* src;       /* (A) */
    const int* dst;       /* (A) ascending */
    const int* label;     /* (A) */
    const int* col;       /* (A) index of label[a] into cols */
    const float* w;       /* (A) */
    const float* final;   /* (Q) -inf: not final */
    const int* cols;      /* (U) the distinct labels, ascending */
    int U;
} oe_decoding_graph;
typedef struct oe_ctc_graph_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_decoding_graph* graph;
    int normalized, max_trav;
    float* score; int* frames; int* arcs; float* path_logp;
    int* n_trav; int* trav_arc; int* trav_start; int* trav_end; float* trav_logp;
    void* workspace;
} oe_ctc_graph_args;
size_t oe_ctc_graph_workspace_bytes(int B, int T, int U, int Q, int A);
int oe_ctc_graph(const oe_ctc_graph_args* args, void* stream);

/* Beam-pruned CTC decoding over large token graphs on device: oe_ctc_graph's recursion by token passing.  The state lives in
 * global memory, the states alive after a frame are kept in an active list, and a beam prunes them: a lexicon loop of 10^5
 * words, a phrase book, a small bigram grammar (what WeNet users mean by TLG decoding).
 *   oe_ctc_graph's, statement for statement: the graph, the node states n[q] and arc states r[a], lp, Tb and the clamping of
 *   labels and indices; the tie rule and the end rule; and the arithmetic - per node q the two best incoming values of frame
 *   t-1 (v1 with its arc id1 and label c1: the best r[a'] into q, lowest id on ties; v2, id2: the best among the arcs whose
 *   label is not c1), m1 = best(n_{t-1}[q], v1), m2 = best(n_{t-1}[q], v2), the node kept unless the arc is strictly greater;
 *   then n_t[q] = lp[t,0] + m1[q] and r_t[a] = lp[t,label[a]] + best(r_{t-1}[a], m + w[a]), m = m1[src[a]] if
 *   c1[src[a]] != label[a] else m2[src[a]], the stay kept unless m + w[a] is strictly greater: float32, the weight added to the
 *   maximum.
 *   Beam: beam is a float32, >= 0 or +inf.  After the values of frame t are made, for every t < Tb-1: best_t = the maximum over
 *   all node and arc states, thr_t = best_t - beam (one float32 subtraction), and every state with a value < thr_t becomes
 *   unreachable before frame t+1 reads it; a state equal to thr_t survives.  The last frame is not pruned, so pruning never
 *   removes a final state from the end rule.  There is no histogram pruning (it would need a tie order among equal values).
 *   Capacity: the survivors of frame t are the states reachable after frame t and its pruning (after the last frame: every
 *   reachable state); max_active >= 1 is how many of them the call can record per frame.  If the survivor count of some
 *   frame exceeds max_active the utterance overflows: its outputs are those of an infeasible utterance, and nothing is
 *   written out of bounds.
 *   out (device memory): score, frames, arcs, path_logp, n_trav, trav_arc, trav_start, trav_end, trav_logp as oe_ctc_graph, and
 *        status (B) int32 = OE_CTC_GRAPH_BEAM_OK (0): decoded;  OE_CTC_GRAPH_BEAM_INFEASIBLE (1): Tb == 0 or no final state
 *        reachable, which pruning may have caused;  OE_CTC_GRAPH_BEAM_OVERFLOW (2);
 *        peak (B) int32 = the largest per-frame survivor count seen (0 for Tb == 0) or, on overflow, the count at the first
 *        overflowing frame, so that a caller can size a retry.
 *   Every output is bit-identical from run to run and those of utterance b depend on utterance b alone; the order in which
 *   threads append to an active list reaches no output (positions in a list are internal; an arg-max over a list breaks
 *   ties by state id).
 *   With beam = +inf, max_active >= Q + A and a graph inside oe_ctc_graph's limits every shared output equals oe_ctc_graph's
 *   bit for bit, on continuous raw logits too.
 *   The graph is one struct, oe_beam_graph: the tables of oe_decoding_graph and the out-adjacency, a CSR of the arcs leaving
 *   each node: out_ptr (Q+1), out_arc (A) = the arc ids ordered by (src, id); host memory read during the call only, its
 *   pointers device pointers (openeat_amd/utils/decoding_graph.py).  The kernel walks arcs forward from the alive states
 *   (out_ptr / out_arc) and pushes arc values to their dst; it does not read in_ptr or src.
 *   Limits: 1 <= B, 1 <= T <= 2^20, V > 1, ldv >= V, 1 <= U < V, max_trav >= 1, max_active >= 1, beam >= 0 (+inf allowed),
 *   1 <= Q <= OE_CTC_GRAPH_BEAM_MAX_NODES, 1 <= A <= OE_CTC_GRAPH_BEAM_MAX_ARCS.  Anything else, and any NULL required
 *   pointer (logits, hlens, graph and its ten tables, score, frames, arcs, n_trav, trav_arc, trav_start, trav_end, status, peak,
 *   workspace), is reported through oe_last_error before any launch, with the outputs untouched.
 *   workspace: oe_ctc_graph_beam_workspace_bytes(B,T,U,Q,A,max_active) bytes, 16-byte aligned (0 for shapes outside the
 *   limits).  With M = min(max_active, Q + A) and Q', A', M' = Q, A, M rounded up to a multiple of 4:
 *     ceil16(4 * B * T * (U + 1))  the lp rows of oe_ctc_kws
 *     + B * (40 * Q'               per node: two 8-byte push keys, value, stamp, touch stamp, list position; a candidate slot
 *            + 20 * A'             per arc: value, stamp, list position; a candidate slot
 *            + 28 * M'             per frame, reused: the touched nodes, the wide ones, and the touched nodes' m1 m2 c1 and the
 *                                  list positions behind m1 and m2
 *            + 8 * T * M')         per frame, kept: state id and back-pointer (a position in the previous frame's list) of each
 *                                  survivor
 *   No T * Q or T * A term: the graph's size is paid once per utterance (the stamps and keys are zeroed once and are
 *   afterwards reset by walking the lists), a frame costs O(survivors + their out-arcs).  Utterances are independent, so a
 *   caller short of memory runs them in groups.
 * Two launches (the row pass of oe_ctc_kws; one workgroup per utterance).  No workgroup waits for another, no float atomics
 * (64-bit integer atomicMax on a packed (order-preserving value, inverted arc id) key keeps the tie rule under the push); no
 * allocation, no host read, no host-side state: capturable. */
#define OE_CTC_GRAPH_BEAM_MAX_NODES (1 << 20)
#define OE_CTC_GRAPH_BEAM_MAX_ARCS (1 << 22)
#define OE_CTC_GRAPH_BEAM_OK 0
#define OE_CTC_GRAPH_BEAM_INFEASIBLE 1
#define OE_CTC_GRAPH_BEAM_OVERFLOW 2
typedef struct oe_beam_graph {
    int Q, A;
    const int* in_ptr;    /* (Q+1) the arcs into q are in_ptr[q] .. in_ptr[q+1]-1 */
    const int* src;       /* (A) */
    const int* dst;       /* (A) ascending */
    const int* label;     /* (A) */
    const int* col;       /* (A) index of label[a] into cols */
    const float* w;       /* (A) */
    const float* final;   /* (Q) -inf: not final */
    const int* cols;      /* (U) the distinct labels, ascending */
    int U;
    const int* out_ptr;   /* (Q+1) the arcs leaving q are out_arc[out_ptr[q] .. out_ptr[q+1]-1] */
    const int* out_arc;   /* (A) arc ids ordered by (src, id) */
} oe_beam_graph;
typedef struct oe_ctc_graph_beam_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_beam_graph* graph;
    int normalized, max_trav, max_active;
    float beam;
    float* score; int* frames; int* arcs; float* path_logp;
    int* n_trav; int* trav_arc; int* trav_start; int* trav_end; float* trav_logp;
    int* status; int* peak;
    void* workspace;
} oe_ctc_graph_beam_args;
size_t oe_ctc_graph_beam_workspace_bytes(int B, int T, int U, int Q, int A, int max_active);
int oe_ctc_graph_beam(const oe_ctc_graph_beam_args* args, void* stream);

/* N-best grammar-constrained CTC decoding on device: the K best DISTINCT paths of the CTC posteriors through a token graph,
 * each with the score of its best alignment - the first pass of a two-pass decode (WeNet takes the n-best of its TLG lattice
 * and rescores them with the decoder).  These are the semantics every layer refers to.
 *   oe_ctc_graph's, statement for statement: the graph struct oe_decoding_graph, the node states n[q] and arc states r[a], lp,
 *   Tb = hlens[b] held to [0, T], normalized, the clamping of labels and indices, and float32 arithmetic.
 *   A state holds an ordered list of at most K tokens, K = nbest, 1 <= K <= OE_CTC_GRAPH_NBEST_MAX, instead of one value.  A
 *   token is (value, history); the history is the sequence of arcs traversed so far, the arc of an arc state included.  Before
 *   frame 0, n[0] holds one token (0, the empty history); every other list is empty.
 *   select_K of an ordered candidate list: sort stably by value, descending (among equal values the earlier candidate comes
 *   first); walk the sorted list, skipping a candidate whose history equals that of a candidate already taken; stop after K.
 *   An unreachable token (value -inf) is never a candidate.
 *   For t = 0 .. Tb-1:
 *     node q: the candidates are the tokens of n_{t-1}[q] in slot order, then, for every arc a' with dst[a'] == q by ascending
 *       id, the tokens of r_{t-1}[a'] in slot order.  n_t[q] = select_K of them, with lp[t,0] added to every value.
 *     arc a, s = src[a]: E = select_K of the tokens of n_{t-1}[s], then the tokens of r_{t-1}[a'] for every a' into s by
 *       ascending id whose col differs from col[a] (the filter comes before the duplicate removal: a history that sits in a
 *       same-label arc and in the node is still a candidate through the node).  The candidates of a are the stay tokens of
 *       r_{t-1}[a] in slot order, then, for each E_k in order, (E_k.value + w[a], E_k.history followed by a).  r_t[a] =
 *       select_K of them, with lp[t,label[a]] added to every value.  The weight is added after the selection of E, as
 *       oe_ctc_graph adds it to the maximum.
 *   End: the candidates are, for q ascending with final[q] > -inf, the tokens of n_{Tb-1}[q] with final[q] added, then, for a
 *   ascending with final[dst[a]] > -inf, the tokens of r_{Tb-1}[a] with final[dst[a]] added; the hypotheses are select_K of
 *   them.  Tb == 0 or no final state reachable: zero hypotheses.
 *   distinct = OE_CTC_GRAPH_NBEST_ARCS (0): histories are arc sequences, the hypotheses are distinct paths.
 *   distinct = OE_CTC_GRAPH_NBEST_TOKENS (1): a history is the sequence of the arcs' cols, the hypotheses are distinct token
 *   sequences, each reporting the arcs of the best path that spells it (parallel arcs of one label and non-deterministic
 *   branches collapse): the mode rescoring wants.
 *   Two histories that differ at a state still differ after the same suffix, so the per-state lists lose nothing: up to float32
 *   rounding the result is the K best distinct paths the graph accepts within Tb frames, each with the score of its best
 *   alignment.  With nbest = 1 the arithmetic is oe_ctc_graph's own: hyp_score[:, 0] equals its score bit for bit and
 *   hyp_arcs[:, 0] its traversal list, on continuous raw logits too.
 *   History identity on the device is a 64-bit hash carried in the token: the empty history is 0, and appending id (the arc,
 *   or its col) is h' = fin(h + 0x9E3779B97F4A7C15 * (id + 1)), fin the splitmix64 finaliser (full avalanche).  Two different
 *   histories compare equal with probability about 2^-64 per comparison.  No output depends on a hash's value: ties are broken
 *   by candidate order only.
 *   Path recovery: every token carries the id of the record of its last "enter an arc" event; a record is the slot (t, a, k) of
 *   a dense table of T*A*K int32 holding the parent record, the arc read off the id; after the end rule one thread per
 *   hypothesis walks the chain.  Alignments of the hypotheses are not produced: oe_ctc_align, or oe_ctc_graph on the path's
 *   linear chain, gives them.
 *   out (device memory):
 *        n_hyp (B) int32 = the number of hypotheses, 0 .. K;
 *        hyp_score (B, K) float32, non-increasing, weights and final weight included, -inf in unused slots;
 *        hyp_len (B, K) int32 = the number of arcs of the path, which may exceed max_len; -1 in unused slots.  The empty path
 *        (the start node final, every frame blank) is a hypothesis of length 0;
 *        hyp_arcs / hyp_tokens (B, K, max_len) int32 = the first max_len arcs and their labels (label[a] as given), -1 behind.
 *   Limits: 1 <= B, 1 <= T <= 2^20, V > 1, ldv >= V, 1 <= U < V, 1 <= Q <= OE_CTC_GRAPH_MAX_NODES, 1 <= A <=
 *   OE_CTC_GRAPH_MAX_ARCS (any graph the dense search takes), 1 <= nbest <= 8, max_len >= 1, distinct in {0, 1}, T*A*K < 2^31.
 *   Anything else, and any NULL required pointer (logits, hlens, graph and its eight tables, the five outputs, workspace), is
 *   reported through oe_last_error before any launch, with the outputs untouched.
 *   workspace: oe_ctc_graph_nbest_workspace_bytes(B,T,U,Q,A,nbest) bytes, 16-byte aligned (0 for shapes outside the limits).
 *   Tokens are 16 bytes (value, record, hash).  Per utterance: the double-buffered token lists of the arcs and the nodes,
 *   16*K*(2*A + 2*Q); the per-node lists "without the arcs of label c" for at most K labels c, 16*K*K*Q, and their labels,
 *   4*K*Q; the record table, 4*T*A*K; the lp rows of oe_ctc_kws, 4*T*(U+1):
 *     16*B*K*(2*A + 2*Q + K*Q) + 4*B*(K*Q + T*A*K + T*(U+1)), rounded up to 16.
 *   It is the record table that callers feel.  Utterances are independent, so a caller short of memory runs them in groups.
 * Two launches (the row pass of oe_ctc_kws; one workgroup per utterance - 1024 threads, 512 where nbest > 2 - with the token
 * lists in the workspace, where they stay in L2).  No workgroup waits for another, no float atomics; no allocation, no host read, no host-side state:
 * capturable.  Every output is bit-identical from run to run and depends on its own utterance only. */
#define OE_CTC_GRAPH_NBEST_MAX 8
#define OE_CTC_GRAPH_NBEST_ARCS 0
#define OE_CTC_GRAPH_NBEST_TOKENS 1
typedef struct oe_ctc_graph_nbest_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_decoding_graph* graph;
    int normalized, nbest, distinct, max_len;
    int* n_hyp; float* hyp_score; int* hyp_len; int* hyp_arcs; int* hyp_tokens;
    void* workspace;
} oe_ctc_graph_nbest_args;
size_t oe_ctc_graph_nbest_workspace_bytes(int B, int T, int U, int Q, int A, int nbest);
int oe_ctc_graph_nbest(const oe_ctc_graph_nbest_args* args, void* stream);

/* Graph CTC likelihood on device: the sum half of oe_ctc_graph.  logZ = log of the sum, over every path the graph accepts and
 * every CTC alignment of it, of the path's probability times exp(its weights), and its gradient with respect to raw logits
 * (what k2 / WeNet users know as a graph CTC loss; the reference has none).  With normalised posteriors and zero weights
 * exp(logZ) is P(the utterance's labelling is in the grammar), and exp(oe_ctc_graph's score - logZ) is the best path's posterior.
 *   The graph, the node states n[q] and arc states r[a], lp, Tb and the clamping of labels and indices are oe_ctc_graph's; every
 *   "best of" becomes a log-sum-exp (LSE).  Before frame 0, n[0] = 0 and every other state is unreachable; for t = 0 .. Tb-1:
 *     r_t[a] = lp[t,label[a]] + LSE( r_{t-1}[a],  n_{t-1}[src[a]] + w[a],
 *                                    r_{t-1}[a'] + w[a] for every a' with dst[a'] == src[a] and label[a'] != label[a] )
 *     n_t[q] = lp[t,0]        + LSE( n_{t-1}[q],  r_{t-1}[a'] for every a' with dst[a'] == q )
 *     logZ   = LSE( n_{Tb-1}[q] + final[q] over q,  r_{Tb-1}[a] + final[dst[a]] over a )
 *   Parallel arcs of one label are separate paths and both count (the weighted-automaton sum).  Tb == 0 or no final state
 *   reachable: the utterance is infeasible, its logp is -inf exactly and its gradient rows are exact zeros.  On
 *   DecodingGraph.linear(tokens) logZ is the CTC log-likelihood of tokens (oe_ctc_nbest_score's); on a token loop with raw
 *   logits every labelling has one state sequence, so logZ = 0 and the gradient is zero.
 *   Gradient (raw logits only).  beta_{Tb-1}[n q] = final[q], beta_{Tb-1}[r a] = final[dst[a]], and for t = Tb-2 .. 0
 *     beta_t[r a] = LSE( lp[t+1,label a] + beta_{t+1}[r a],  lp[t+1,0] + beta_{t+1}[n dst[a]],
 *                        w[a''] + lp[t+1,label a''] + beta_{t+1}[r a''] for a'' with src[a''] == dst[a], label[a''] != label[a] )
 *     beta_t[n q] = LSE( lp[t+1,0] + beta_{t+1}[n q],  w[a''] + lp[t+1,label a''] + beta_{t+1}[r a''] for a'' with src[a''] == q )
 *   occ[t,v] = the sum over the states s of label v (node states count for v = 0) of exp(alpha_t[s] + beta_t[s] - logZ); each
 *   row of occ sums to 1.  dlogits[b,t,v] = g[b] * (occ[b,t,v] - softmax(logits[b,t,:])[v]) for t < Tb, the gradient of
 *   sum_b g[b] * logp[b]; rows t >= Tb and every row of an infeasible utterance are exact zeros; columns >= V are never
 *   written; g of an infeasible utterance is not read into any result (it may be NaN), as in oe_ctc_nbest_grad.
 *   oe_graph_set: G graphs concatenated (built by openeat_amd/utils/decoding_graph.py, GraphSet; host memory read during the
 *   call only, its pointers device pointers, every table int32 but w and final).  Graph i owns the nodes node_off[i] ..
 *   node_off[i+1]-1 and the arcs arc_off[i] .. arc_off[i+1]-1 of the concatenated tables; every index stored in a table is
 *   local to its graph.  A table of n+1 entries per graph (n = its nodes, arcs or groups) lies at node_off[i] + i or
 *   arc_off[i] + i.  The set has ONE cols / U, the union of its graphs' labels, so one compact lp row serves every utterance.
 *     the tables of oe_decoding_graph: in_ptr (Q+G), src, dst, label, col, w (A), final (Q), cols (U);
 *     in-groups: the arcs into a node ordered by (col, id) are in_perm (A); a group is a maximal run of one col;
 *       in_gptr (Q+G): the groups of node q are in_gptr[q] .. in_gptr[q+1]-1; in_gstart (A+G): group g holds
 *       in_perm[in_gstart[g] .. in_gstart[g+1]-1]; in_xg (A): the in-group of src[a] that carries col[a], or -1;
 *     out-groups, the mirror image over the arcs leaving a node: out_perm, out_gptr, out_gstart, and out_xg (A): the
 *       out-group of dst[a] that carries col[a], or -1;
 *     by column: col_perm (A) the arcs ordered by (col, id), col_ptr (G * (U+1)): graph i's arcs of column k are
 *       col_perm[col_ptr[i*(U+1)+k] .. col_ptr[i*(U+1)+k+1]-1];
 *     inv (n_inv): inv[v] = 0 for v = 0, 1 + k where cols[k] == v, -1 otherwise (a label v >= V takes no gradient);
 *     Q, A the totals, Qmax / Amax the largest graph's.
 *   graph_of (B) int32 on the device names each utterance's graph, held to [0, G); NULL: graph 0 for all.
 *   oe_ctc_graph_logp: logp (B) float32.  workspace: oe_ctc_graph_logp_workspace_bytes(B,T,U,Qmax,Amax) = 4*B*T*(U+1), the lp
 *   rows of oe_ctc_kws; the score keeps no other per-frame state.
 *   oe_ctc_graph_logp_grad: g (B) float32 in; dlogits (B, T, ldv) out, which may not alias logits; logp (B) out or NULL,
 *   bit-identical to oe_ctc_graph_logp's.  normalized != 0 is an error.  It runs the forward recursion itself and keeps alpha in
 *   its workspace - nothing is handed over from the score call, so a caller short of memory runs utterance groups in both
 *   directions with one workspace: oe_ctc_graph_logp_grad_workspace_bytes(B,T,U,Qmax,Amax) = lp and occ rows
 *   (2 * 4*B*T*(U+1)), a row log-sum-exp (4*B*T), logZ (8*B) and alpha (8*B*T*(Qmax+Amax)), each part rounded up to 16 bytes.
 *   Numbers: the state is float64 in the log2 domain with a finite "log 0" (-1e30), exp / log are float32 on differences, the
 *   scheme of oe_ctc_loss_fused above 248 frames; there is no float32 path.  "All arcs into src[a] but those of label[a]" is
 *   never a subtraction: per node a forward sweep over its groups leaves the prefix LSE in a slot per group and a backward sweep
 *   combines the suffix into it (a wave with a log-semiring scan for a node of more than 32 arcs), O(A + Q) per frame.
 *   Against the float64 restatement (tests/ctc_graph_logp_ref.py): logp rtol 1e-4 / atol 1e-3, gradient rtol 2e-3 / atol
 *   2e-5 * |g[b]|, the tolerances of oe_ctc_loss_fused.  Worst observed (tests/test_ctc_graph_logp_gpu.py, one MI355X): 0.0008 of
 *   the logp tolerance and 0.033 of the gradient's (a token loop, V = 300); 0.0002 / 0.0024 at T = 600 with logp = -1724.
 *   Limits: 1 <= B, 1 <= T <= 2^20, V > 1, ldv >= V, 1 <= U < V, 1 <= G, 1 <= Qmax <= OE_CTC_GRAPH_LOGP_MAX_NODES,
 *   1 <= Amax <= OE_CTC_GRAPH_LOGP_MAX_ARCS: one workgroup holds 24 bytes per arc (r, and two values per group) and 8 per node
 *   in the 160 KiB of LDS (24 * 5120 + 8 * 4096 = 152 KiB, the rest its lists and reduction slots).  Anything else, any NULL
 *   required pointer (logits, hlens, set and its tables, logp for the score; g, dlogits for the gradient; workspace), a
 *   workspace not 16-byte aligned, and dlogits == logits are reported through oe_last_error before any launch, with the outputs
 *   untouched.  The size functions return 0 outside the limits.
 * Launches: the row pass of oe_ctc_kws; one workgroup per utterance (score: the forward recursion; gradient: forward, beta and
 * the occupancies); for the gradient one dense pass over the dlogits rows.  Every sum runs in a fixed order: results are
 * bit-identical from run to run, logp[b] and dlogits[b] depend on utterance b alone.  No float atomics, no workgroup waits for
 * another; no allocation, no host read, no host-side state: capturable. */
#define OE_CTC_GRAPH_LOGP_MAX_NODES 4096
#define OE_CTC_GRAPH_LOGP_MAX_ARCS 5120
typedef struct oe_graph_set {
    int G, Q, A, U, Qmax, Amax, n_inv;
    const int* node_off;  /* (G+1) */
    const int* arc_off;   /* (G+1) */
    const int* in_ptr;    /* (Q+G) */
    const int* src;       /* (A) */
    const int* dst;       /* (A) */
    const int* label;     /* (A) */
    const int* col;       /* (A) index of label[a] into cols */
    const float* w;       /* (A) */
    const float* final;   /* (Q) -inf: not final */
    const int* cols;      /* (U) the distinct labels of all graphs, ascending */
    const int* in_gptr;   /* (Q+G) */
    const int* in_gstart; /* (A+G) */
    const int* in_perm;   /* (A) */
    const int* in_xg;     /* (A) */
    const int* out_gptr;  /* (Q+G) */
    const int* out_gstart;/* (A+G) */
    const int* out_perm;  /* (A) */
    const int* out_xg;    /* (A) */
    const int* col_ptr;   /* (G*(U+1)) */
    const int* col_perm;  /* (A) */
    const int* inv;       /* (n_inv) */
} oe_graph_set;
typedef struct oe_ctc_graph_logp_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_graph_set* set;
    const int* graph_of;
    int normalized;
    float* logp;
    void* workspace;
} oe_ctc_graph_logp_args;
typedef struct oe_ctc_graph_logp_grad_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_graph_set* set;
    const int* graph_of;
    int normalized;
    const float* g;
    float* dlogits;
    float* logp;
    void* workspace;
} oe_ctc_graph_logp_grad_args;
size_t oe_ctc_graph_logp_workspace_bytes(int B, int T, int U, int Qmax, int Amax);
size_t oe_ctc_graph_logp_grad_workspace_bytes(int B, int T, int U, int Qmax, int Amax);
int oe_ctc_graph_logp(const oe_ctc_graph_logp_args* args, void* stream);
int oe_ctc_graph_logp_grad(const oe_ctc_graph_logp_grad_args* args, void* stream);

/* Beam-pruned graph CTC likelihood on device over large token graphs: the sum half of oe_ctc_graph_beam.  logZ = the log of the
 * sum over every path of the graph that survives a beam, and its gradient with respect to raw logits: the rejection score, the
 * best-path posterior, the graph loss and the MMI denominator of a lexicon loop of 10^5 words, a phrase book, a bigram grammar -
 * the graphs oe_ctc_graph_logp cannot hold in LDS.  These are the semantics every layer refers to.
 *   Shared: the graph, the node states n[q] and arc states r[a], lp, Tb and the clamping of labels and indices are
 *   oe_ctc_graph's; the recursion is oe_ctc_graph_logp's: every "best of" is a log-sum-exp, parallel arcs both count.
 *   Beam: beam is a float32, >= 0 or +inf.  After the values (alpha) of frame t are made, for every t < Tb-1: best_t = the
 *   maximum over all node and arc values, thr_t = best_t - beam, and every state with alpha < thr_t becomes unreachable before
 *   frame t+1 reads it; a state equal to thr_t survives.  The last frame is not pruned.  S_t = the survivors of frame t.
 *   logZ = LSE over S_{Tb-1} of alpha + final, as in oe_ctc_graph_logp.  (The comparison runs on the kernel's float64 log2-domain
 *   values; a state within rounding of a threshold may fall on either side.)
 *   Capacity, status, peak, overflow: oe_ctc_graph_beam's, word for word, with OE_CTC_GRAPH_BEAM_OK / _INFEASIBLE / _OVERFLOW.
 *   An overflowed or infeasible utterance has logp = -inf exactly and exact-zero gradient rows; its g is never read into a result.
 *   Gradient (raw logits only; normalized != 0 is an error): the derivative of logZ with the survivor sets held fixed, which is
 *   the true derivative wherever no value sits on a threshold.  beta on the sub-lattice: beta_{Tb-1} is oe_ctc_graph_logp's end
 *   rule on S_{Tb-1}; beta_t[s] for s in S_t sums only over successors in S_{t+1}; beta_t[s] = "log 0" for s not in S_t.
 *   occ[t,v] = the sum over the states of label v in S_t of exp(alpha + beta - logZ); each occ row sums to 1 (a float64
 *   restatement measured row-sum errors <= 3e-14).  dlogits = g[b] * (occ - softmax) for t < Tb; rows t >= Tb are exact zeros;
 *   columns >= V are never written.
 *   With beam = +inf, max_active >= Q + A and a graph inside oe_ctc_graph_logp's limits, logp and dlogits agree with
 *   oe_ctc_graph_logp and oe_ctc_graph_logp_grad within the tolerances below - not bit for bit: the arithmetic differs.
 *   Every output is bit-identical from run to run and those of utterance b depend on utterance b alone; the order in which
 *   threads append to a list reaches no output.
 *   oe_ctc_graph_beam_logp: logp (B) float32, status (B), peak (B) int32 out.  oe_ctc_graph_beam_logp_grad: g (B) float32 in;
 *   dlogits (B, T, ldv) out, which may not alias logits; status, peak out; logp (B) out or NULL, bit-identical to the score
 *   call's.  It runs the forward sweep itself; nothing is handed over from the score call.
 *   The graph is one struct, oe_beam_logp_graph: the tables of oe_beam_graph and the label groups the sum needs, per arc
 *   (openeat_amd/utils/decoding_graph.py builds them once on the host; group ids are those of oe_graph_set for a set of this
 *   one graph): in_grp (A) = the in-group of dst[a] that holds a; out_grp (A) = the out-group of src[a] that holds a; in_xg,
 *   out_xg (A) as in oe_graph_set; inv (n_inv) as in oe_graph_set.  Host memory read during the call only, its pointers device
 *   pointers.
 *   Numbers: the state is float64 in the log2 domain with a finite "log 0", exp / log float32 on differences, as in
 *   oe_ctc_graph_logp.  A sum over the arcs into a node is pushed by many threads and must not depend on their order: per
 *   touched node v1 / c1 (the greatest incoming value up to a float32 rounding, its label) and v2 (likewise among the arcs of
 *   another label than c1) by 64-bit integer atomicMax on oe_ctc_graph_beam's keys; then every alive incoming arc adds
 *   exp2(v - v1) as a 64-bit fixed-point integer at scale 2^40 to a per-node total S1 and, if its label is not c1, to its
 *   (node, label) group slot G and exp2(v - v2) to S2.  Integer adds are associative; 2^22 terms of at most 2^41 cannot
 *   overflow.  "Every incoming arc of another label" for a leaving arc of label c is S2 (scaled by v2) if c == c1, else the
 *   exact integer difference S1 - G[c], which always contains v1's term: never a cancellation, the sum of the other groups to
 *   2^-40 of the largest.  beta is the mirror image over the out-groups; the occupancies add as fixed-point integers into a
 *   row of U + 1 per frame; logZ is a maximum over the last list and one more fixed-point sum.
 *   Against the float64 restatement (tests/ctc_graph_beam_logp_ref.py): oe_ctc_graph_logp's tolerances, logp rtol 1e-4 / atol
 *   1e-3, gradient rtol 2e-3 / atol 2e-5 * |g[b]|.  Worst observed (tests/test_ctc_graph_beam_logp_gpu.py, one MI355X): 0.0008
 *   of the logp tolerance and 0.042 of the gradient's (a token loop, V = 300, beam = inf); with a beam 0.0008 / 0.0097 (a
 *   lexicon loop of 5403 nodes and 10402 arcs, beams 10 and 14).  A pruned comparison is discrete - a state within rounding
 *   of a threshold may fall on either side - so the tests compare where the restatement is insensitive to the beam.
 *   Limits: B, T, V, ldv, U, max_active and beam as in oe_ctc_graph_beam; 1 <= Q <= OE_CTC_GRAPH_BEAM_MAX_NODES, 1 <= A <=
 *   OE_CTC_GRAPH_BEAM_MAX_ARCS.  Anything else, any NULL required pointer (logits, hlens, graph and its tables - inv may be
 *   NULL where n_inv == 0 -, logp for the score, g and dlogits for the gradient, status, peak, workspace), a workspace not
 *   16-byte aligned, and dlogits == logits are reported through oe_last_error before any launch, with the outputs untouched.
 *   The size functions return 0 outside the limits.
 *   workspace, 16-byte aligned.  With M = min(max_active, Q + A), Q', A', M', T' = Q, A, M, T rounded up to a multiple of 4 and
 *   R = ceil16(4 * B * T * (U + 1)), the lp rows of oe_ctc_kws:
 *   oe_ctc_graph_beam_logp_workspace_bytes(B,T,U,Q,A,max_active) =
 *     R + B * (52 * Q'   per node: two push keys, S1, S2 (8 each), value (8), stamp, touch stamp, a candidate slot (4 each)
 *            + 24 * A'   per arc: group slot G (8), value (8), stamp, a candidate slot
 *            + 60 * M')  per frame, reused: the touched nodes, the wide ones, five 8-byte aggregates and c1 per touched node,
 *                        and two active lists of state ids used in turn
 *   oe_ctc_graph_beam_logp_grad_workspace_bytes(B,T,U,Q,A,max_active) =
 *     3 * R              the lp rows, and the occupancy rows as 64-bit fixed point
 *     + ceil16(4 * B * T) + ceil16(8 * B)   the rows' log-sum-exp, logZ
 *     + B * (64 * Q' + 36 * A'   as above, and beta with its stamp per node and per arc
 *            + 60 * M'           as above, with a buffer of new betas in place of the two lists
 *            + 4 * T'            the survivor count of each frame
 *            + 12 * T * M')      per frame, kept: state id and alpha of each survivor
 *   No T * Q or T * A term: the graph's size is paid once per utterance, a frame costs O(survivors + their out-arcs) - a hub's
 *   in-arcs are never walked.  Utterances are independent, so a caller short of memory runs them in groups.
 * Launches: the row pass of oe_ctc_kws; one workgroup of 1024 threads per utterance (score: the forward sweep; gradient:
 * forward, the backward sweep over the stored lists, the occupancies); for the gradient one dense pass over the dlogits rows.
 * No workgroup waits for another, no float atomics; no allocation, no host read, no host-side state: capturable. */
typedef struct oe_beam_logp_graph {
    int Q, A;
    const int* in_ptr;    /* (Q+1) the arcs into q are in_ptr[q] .. in_ptr[q+1]-1 */
    const int* src;       /* (A) */
    const int* dst;       /* (A) ascending */
    const int* label;     /* (A) */
    const int* col;       /* (A) index of label[a] into cols */
    const float* w;       /* (A) */
    const float* final;   /* (Q) -inf: not final */
    const int* cols;      /* (U) the distinct labels, ascending */
    int U;
    const int* out_ptr;   /* (Q+1) the arcs leaving q are out_arc[out_ptr[q] .. out_ptr[q+1]-1] */
    const int* out_arc;   /* (A) arc ids ordered by (src, id) */
    const int* in_grp;    /* (A) the in-group of dst[a] that holds a */
    const int* in_xg;     /* (A) the in-group of src[a] that carries col[a], or -1 */
    const int* out_grp;   /* (A) the out-group of src[a] that holds a */
    const int* out_xg;    /* (A) the out-group of dst[a] that carries col[a], or -1 */
    const int* inv;       /* (n_inv) */
    int n_inv;
} oe_beam_logp_graph;
typedef struct oe_ctc_graph_beam_logp_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_beam_logp_graph* graph;
    int normalized, max_active;
    float beam;
    float* logp; int* status; int* peak;
    void* workspace;
} oe_ctc_graph_beam_logp_args;
typedef struct oe_ctc_graph_beam_logp_grad_args {
    const float* logits; long ldv; int B, T, V;
    const int* hlens;
    const oe_beam_logp_graph* graph;
    int normalized, max_active;
    float beam;
    const float* g;
    float* dlogits;
    float* logp; int* status; int* peak;
    void* workspace;
} oe_ctc_graph_beam_logp_grad_args;
size_t oe_ctc_graph_beam_logp_workspace_bytes(int B, int T, int U, int Q, int A, int max_active);
size_t oe_ctc_graph_beam_logp_grad_workspace_bytes(int B, int T, int U, int Q, int A, int max_active);
int oe_ctc_graph_beam_logp(const oe_ctc_graph_beam_logp_args* args, void* stream);
int oe_ctc_graph_beam_logp_grad(const oe_ctc_graph_beam_logp_grad_args* args, void* stream);

/* ------------------------------------------------------------------------- *
 * Fused multi-head attention (scores -> mask -> softmax -> 0-fill -> dropout
 * -> .V), forward and backward, for attention.py:65-97,112-117,189-209.
 *   q (B,T1,H,D), k/v (B,T2,H,D), out (B,T1,H,D): element (b,t,h,d) at
 *   base + b*bstride + t*rstride + h*D + d (so q/k/v may be slices of one
 *   fused projection buffer).  D <= 64.
 *   mask: bytes, (b,i,j) at mask + b*mask_bstride + i*mask_rstride + j;
 *         mask_rstride = 0 for a (B,1,T2) key mask.  0 = masked out.  Rows
 *         with no valid key produce zeros (the reference's 0-fill).
 *   keybias (B,H,T2): added to the scaled score (relative-position term,
 *         see oe_relpos_prepare); NULL for plain attention.
 *   scores = scale * q.k + keybias;  lse (B,H,T1) natural-log normaliser.
 *   dropout acts on the normalised weights, index ((b*H+h)*T1+i)*T2+j.
 * backward: needs out, lse, d_out; writes dq, dk, dv (same strides as q,k,v),
 *   dkeybias (B,H,T2) if keybias was given; delta (B,H,T1) is scratch.
 * ------------------------------------------------------------------------- */
typedef struct oe_attn_args {
    const float* q; long q_bstride, q_rstride;
    const float* k; long k_bstride, k_rstride;
    const float* v; long v_bstride, v_rstride;
    float* out; long o_bstride, o_rstride;
    float* lse;
    const unsigned char* mask; long mask_bstride, mask_rstride;
    const float* keybias;
    int B, H, T1, T2, D;
    float scale;
    float drop_p; unsigned long long seed; const unsigned long long* seed_dev;
    /* backward only */
    const float* d_out;
    float* dq; float* dk; float* dv;
    float* dkeybias;
    float* delta;
    /* matrix-core arithmetic of the score / context products, as oe_gemm_args.precision:
     * 0 = fp32 MFMA (exact products), 1 = bf16 inputs, 3 = three-term bf16 split (2^-17 per product),
     * 6 = six terms on three exact bf16 pieces (fp32-MFMA-grade) */
    int precision;
    /* hint, forward: the (B, T1, T2) mask is zero above the diagonal (a decoder's self-attention): key blocks that lie wholly
     * above it are not visited.  Results are identical with or without the hint; ignored unless a full mask is given. */
    int causal;
} oe_attn_args;

int oe_attention_fwd(const oe_attn_args* args, void* stream);
int oe_attention_bwd(const oe_attn_args* args, void* stream);

/* Relative-position attention preparation (attention.py:185-200 without
 * rel_shift):  kp[b,t,h,:] = k[b,t,h,:] + p[t,h,:]  (dense (B,T,H,D)),
 * keybias[b,h,t] = scale*(u_h . k[b,t,h,:] + v_h . p[t,h,:]).
 * k: element (b,t,h,d) at k + b*k_bstride + t*k_rstride + h*D + d; p = linear_pos(pos_emb), row stride p_rstride. */
int oe_relpos_prepare(const float* k, long k_bstride, long k_rstride, const float* p, long p_rstride,
                      const float* u, const float* v, int B, int T, int H, int D, float scale, float* kp,
                      float* keybias, void* stream);
/* backward of the above: dk (k's strides) written, dp (T,H,D; row stride
 * dp_rstride) written, du/dv (H,D) accumulated atomically. */
int oe_relpos_backward(const float* dkp, const float* dkeybias, const float* k, long k_bstride, long k_rstride,
                       const float* p, long p_rstride, const float* u, const float* v, int B, int T, int H, int D,
                       float scale, float* dk, float* dp, long dp_rstride, float* du, float* dv, void* stream);

/* GLU over channels, a (rows, 2d) -> y (rows, d)  (convolution.py:104). */
int oe_glu_fwd(const float* a, long rows, int d, float* y, void* stream);
int oe_glu_bwd(const float* a, const float* dy, long rows, int d, float* da, void* stream);

/* out[i] = alpha * x[i] * dropmask(seed, i)/(1-p); rows (of `cols`) with
 * rowmask==0 -> 0.  Backward of the dropout/mask epilogues (torch.nn.Dropout in
 * encoder_layer.py:83,89,95,106 and decoder_layer.py:92,97,106). */
int oe_dropout_scale(const float* x, long n, int cols, float alpha, float p, unsigned long long seed,
                     const unsigned long long* seed_dev, const unsigned char* rowmask, float* out, void* stream);

/* Token embedding * sqrt(d) + positional table (decoder.py:144-147 +
 * embedding.py:59): out[r,:] = table[tok[r],:]*xscale + pe[r % L,:]; backward
 * accumulates into dtable atomically. tokens int64. */
int oe_embed_fwd(const long long* tokens, const float* table, const float* pe, long rows, int L, int d, int V,
                 float xscale, float* out, void* stream);
int oe_embed_bwd(const long long* tokens, const float* dout, long rows, int d, int V, float xscale, float* dtable,
                 void* stream);

/* in [A][B][C] -> out [A][C][B] (optionally accumulated): weight layout change
 * between the checkpoint layout (subsampling.py:79 OIHW, :113 channel-major
 * flatten) and the NHWC kernels. */
int oe_swap_last2(const float* in, long A, int Bd, int Cd, float* out, int accumulate, void* stream);
/* Helpers of the input gradient of a stride-2 3x3 NHWC convolution done as four stride-1 implicit GEMMs, one per parity
 * class of the input position (the backward of subsampling.py:110-116's second Conv2d):
 * oe_pad1_nhwc: dy (B, To, Fo, C) -> out (B, To+2, Fo+2, C) with a border of zeros (C % 4 == 0, 16-byte aligned);
 * oe_conv_dgrad_k3s2_weights: OIHW weight w[C][C][3][3] -> the four classes' B operands [ci][(window row, window col, co)]
 * back to back in out (9 C^2 floats; class (t1%2, f1%2) at offsets 0, 4C^2, 6C^2, 8C^2). */
int oe_pad1_nhwc(const float* dy, int B, int To, int Fo, int C, float* out, void* stream);
/* oe_pad1_nhwc straight into three bf16 planes of the padded tensor (plane n at planes + n * plane_stride elements, rows of C;
 * oe_split_planes' definition); out (the padded fp32 tensor) is optional - the parity-class GEMMs on pre-split operands read
 * the planes only. */
int oe_pad1_nhwc_planes(const float* dy, int B, int To, int Fo, int C, float* out, void* planes, long plane_stride, void* stream);
int oe_conv_dgrad_k3s2_weights(const float* w, int C, float* out, void* stream);

/* The joint loss of /root/reference/openeat/models/asr_model.py:150-157 and :196-198 as one launch on device scalars:
 *   att = loss_att * (1 - reverse_weight) + loss_att_r * reverse_weight   (loss_att_r NULL: att = loss_att)
 *   out = (ctc_weight * loss_ctc + (1 - ctc_weight) * att) * inv_accum    (loss_ctc NULL: out = att * inv_accum)
 * each product and sum rounded on its own in that order (the value torch's scalar ops produce); oe_loss_combine_bwd writes
 * the three gradients for an incoming scalar gradient g (d_ctc / d_att_r NULL where the term is absent). */
int oe_loss_combine(const float* loss_ctc, const float* loss_att, const float* loss_att_r, float ctc_weight, float reverse_weight,
                    float inv_accum, float* out, void* stream);
int oe_loss_combine_bwd(const float* g, float ctc_weight, float reverse_weight, float inv_accum, float* d_ctc, float* d_att,
                        float* d_att_r, void* stream);

/* out = a*(*a_dev)*x + b*y (y, a_dev may be NULL). */
int oe_axpby(const float* x, const float* y, long n, float a, float b, const float* a_dev, float* out, void* stream);

/* y = act(x) (swish.py:15-17) and out = dy * act'(pre). */
int oe_act_fwd(const float* x, long n, int act, float* y, void* stream);
int oe_act_grad(const float* dy, const float* pre, long n, int act, float* out, void* stream);

/* log_softmax over the last dim (ctc.py:56-64; asr_model.py:484-488). */
int oe_log_softmax(const float* x, long rows, int V, float* out, void* stream);
/* log_softmax(x)[row, idx_a[row]] (0 where idx_a is out of range) and, if out_b is given, log_softmax(x)[row, idx_b] for one
 * fixed column - the hypothesis' token and <eos> log-probabilities attention rescoring sums (asr_model.py:504-528) - without
 * writing the (rows, V) log-probability tensor. */
int oe_logprob_gather(const float* x, long rows, int V, const long long* idx_a, int idx_b, float* out_a, float* out_b, void* stream);
/* The decoders' token bookkeeping of a training step in one launch (asr_model.py:162-176 with common.py:61-132 and
 * mask.py:9-69): from the labels ys_pad (B, L) i32 (ignore_id where there is none) and their lengths (B) i32, at the fixed
 * width W = L + 1: ys_in = [sos, labels, eos...], ys_out = [labels, eos, ignore...] (both (B, W) i64), the same for the
 * reversed labels (r_ys_in / r_ys_out, or both NULL), and tgt_mask (B, W, W) u8 = (j < len + 1) && (j <= i). */
int oe_att_inputs(const int* ys_pad, const int* ys_lens, int B, int L, int sos, int eos, int ignore_id, long long* ys_in,
                  long long* ys_out, long long* r_ys_in, long long* r_ys_out, unsigned char* tgt_mask, void* stream);
/* Per-row top-k, sorted descending, of x (rows, V) or - log_softmax != 0 - of its row-wise log-softmax, fused
 * (asr_model.py:251, 358 `log_softmax(...).topk(beam_size)`; :258 `scores.topk`).  vals (rows, k) f32, idx (rows, k) i64;
 * ties go to the lowest index.  k <= V <= 40000. */
int oe_topk_rows(const float* x, long rows, int V, int k, int log_softmax, float* vals, long long* idx, void* stream);

/* Masked softmax (+ dropout) over the last dim of a MATERIALISED score tensor: the module-API method
 * MultiHeadedAttention.forward_attention (attention.py:65-97) - the training / decoding path never builds this tensor
 * (oe_attention_fwd).  scores (B,H,T1,T2) dense; mask bytes (b,i,j) at mask + b*mask_bstride + i*mask_rstride + j
 * (mask_rstride = 0: a (B,1,T2) key mask; NULL: no mask), 0 = masked: -inf before the softmax, 0 after it
 * (attention.py:85-88).  y = the softmax (kept for backward), out = y * dropout(drop_p, element index) (out may alias y
 * when drop_p == 0).  backward: dscores = y * (g - sum_j g_j y_j), g = dout * the same dropout mask; rows = B*H*T1. */
int oe_masked_softmax_fwd(const float* scores, const unsigned char* mask, long mask_bstride, long mask_rstride, int B, int H,
                          int T1, int T2, float drop_p, unsigned long long seed, const unsigned long long* seed_dev, float* y,
                          float* out, void* stream);
int oe_masked_softmax_bwd(const float* y, const float* dout, long rows, int T2, float drop_p, unsigned long long seed,
                          const unsigned long long* seed_dev, float* dscores, void* stream);

/* GlobalCMVN (modules/cmvn.py:43-45): y = (x - mean[f]) * istd[f]. */
int oe_global_cmvn(const float* x, const float* mean, const float* istd, long n, int F, float* y, void* stream);

/* Conv2d(1,C,3,stride 2)+ReLU of the subsampling front (subsampling.py:77-78):
 * x (B,T,F) -> y (B,T1,F1,C) NHWC, w (C,1,3,3).  wgrad: dy must already be
 * masked by y>0; dw/db accumulated atomically. */
int oe_conv1_fwd(const float* x, const float* w, const float* bias, int B, int T, int F, int C, float* y, void* stream);
/* the same, also writing y as three bf16 planes (oe_split_planes' layout: plane n at y_planes + n * plane_stride elements, rows of C)
 * for a precision-6 conv2 on pre-split operands; y_planes NULL = oe_conv1_fwd; y NULL (with y_planes): the planes are the only
 * copy written (oe_gemm_args.actgrad_bf16 reads the ReLU mask from plane 0) */
int oe_conv1_fwd_pl(const float* x, const float* w, const float* bias, int B, int T, int F, int C, float* y,
                    void* y_planes, long plane_stride, void* stream);
int oe_conv1_wgrad(const float* x, const float* dy, int B, int T, int F, int C, float* dw, float* db, void* stream);

/* Input gradient of Conv2d(C,C,3,stride 2) in gather form, fused with the
 * ReLU mask of the layer below (autograd of subsampling.py:78-79):
 * dcol (B*T2*F2, 9C) = dy @ W[co][kh][kw][ci]  ->  dx (B,T1,F1,C) * (y1 > 0). */
int oe_col2im_relu(const float* dcol, const float* y1, int B, int T1, int F1, int C, float* dx, void* stream);
/* the same for a KS x KS kernel with stride S (oe_col2im_relu = 3, 2) */
int oe_col2im_relu_ks(const float* dcol, const float* y1, int B, int T1, int F1, int C, int KS, int S, float* dx,
                      void* stream);

/* GLU + depthwise Conv1d(K, groups=d) of the Conformer conv module
 * (convolution.py:104-107): a (B,T,2d) -> y (B,T,d); w (d,1,K); causal => left
 * padding K-1 (convolution.py:40-47,92-93).  gpad (optional, [d]): value of the
 * GLU output on the virtual frames t < 0 - the reference pads BEFORE the
 * pointwise conv, so they carry GLU(pointwise bias); dgpad accumulates its
 * gradient.  backward: da (B,T,2d) written, dw/db accumulated atomically. */
int oe_dwconv_glu_fwd(const float* a, const float* w, const float* bias, const float* gpad, int B, int T, int d,
                      int K, int causal, float* y, void* stream);
/* oe_dwconv_glu_fwd plus the LayerNorm + activation that follows it in the Conformer convolution module
 * (/root/reference/openeat/modules/convolution.py:107-111) from the same launch: z (optional) = act(LN(y)), ln_stats = (mean, rstd)
 * per row as oe_layernorm_fwd writes them; bit-identical to oe_dwconv_glu_fwd followed by oe_layernorm_fwd. */
int oe_dwconv_glu_ln_fwd(const float* a, const float* w, const float* bias, const float* gpad, int B, int T, int d, int K, int causal,
                         float* y, const float* ln_gamma, const float* ln_beta, float ln_eps, int ln_act, float* z, float* ln_stats,
                         void* stream);
size_t oe_dwconv_glu_bwd_workspace_floats(int B, int T, int d, int K);
int oe_dwconv_glu_bwd(const float* a, const float* dy, const float* w, const float* gpad, int B, int T, int d, int K,
                      int causal, float* da, float* dw, float* db, float* dgpad, float* workspace, void* stream);

/* Label-smoothed KL loss + accuracy + gradient, fused
 * (label_smoothing_loss.py:58-91, common.py:135-157).  logits (rows, ldv) are
 * OVERWRITTEN by grad_scale/denom * (softmax - true_dist) when write_grad;
 * rows with target == ignore_id give 0.  denom = batch_size, or the number of
 * non-ignored rows when normalize_length.  out3 = {loss, #correct, #valid}.
 * target int64.  workspace: oe_lsm_workspace_bytes(rows). */
size_t oe_lsm_workspace_bytes(long rows);
int oe_lsm_loss_fused(float* logits, long ldv, long rows, int V, const long long* target, int ignore_id, float smoothing,
                      int normalize_length, float batch_size, float grad_scale, int write_grad, float* out3,
                      void* workspace, void* stream);

/* Global L2 norm of the flat gradient arena (clip_grad_norm_, executor.py:58). */
size_t oe_grad_norm_workspace_floats(void);
int oe_grad_norm(const float* g, long n, float* workspace, float* norm_out, void* stream);
/* clip + Adam over the flat arenas (torch.optim.Adam defaults; executor.py:59-61:
 * the step is skipped when the norm is not finite).  state: float[2] device,
 * state[0] = step count, state[1] = 0.  lr_dev (device scalar) overrides lr. */
int oe_adam_step(float* p, const float* g, float* m, float* v, long n, const float* lr_dev, float lr, float beta1,
                 float beta2, float eps, float max_norm, const float* total_norm, float* state, void* stream);

/* Kaldi log-mel filterbank on device, replacing the torchaudio.compliance.kaldi.fbank
 * call of dataset.py:93-100 (frame_length 25 ms, frame_shift 10 ms, snip_edges,
 * remove_dc_offset, preemphasis 0.97, povey window, power spectrum, 20 Hz..Nyquist
 * mel triangles, log with FLT_EPSILON floor) incl. the x 2^15 of dataset.py:75.
 *   wav (B, wav_stride) float; nsamples (B) valid samples per row or NULL (= wav_stride)
 *   out (B, Tmax, n_mel); frames beyond 1+(n-win)/hop are written as 0.
 *   window [win]; twiddle [256][2] = (cos, -sin)(2 pi k/512); mel filter m covers FFT bins
 *   mel_start[m] .. with weights mel_w[mel_off[m] .. mel_off[m+1]).
 *   cmvn_mean/istd (optional, [n_mel]): GlobalCMVN (modules/cmvn.py:43-45) fused in. */
int oe_fbank(const float* wav, const int* nsamples, int B, long wav_stride, int Tmax, int win, int hop, int n_mel,
             float scale, float preemph, const float* window, const float* twiddle, const int* mel_start,
             const int* mel_off, const float* mel_w, float floor_eps, const float* cmvn_mean,
             const float* cmvn_istd, float* out, void* stream);
/* The same with kaldi's waveform dither (dataset.py:98, `dither=wav_dither`): N(0, dither^2) noise on every sample of every
 * frame's window (after the x 2^15), drawn from a counter-based generator keyed by (seed, frame, sample).  Distribution
 * parity with the reference (torch's global generator there), not bit parity.  dither = 0 is oe_fbank. */
int oe_fbank_dither(const float* wav, const int* nsamples, int B, long wav_stride, int Tmax, int win, int hop, int n_mel,
                    float scale, float preemph, const float* window, const float* twiddle, const int* mel_start,
                    const int* mel_off, const float* mel_w, float floor_eps, const float* cmvn_mean,
                    const float* cmvn_istd, float dither, unsigned long long seed, float* out, void* stream);
/* Per-utterance (x - mean_t)/std_t over each utterance's own nframes[b] frames, in place
 * (feature_processor.py:5-8: population std, no epsilon). */
int oe_utt_normalize(float* x, const int* nframes, int B, int Tmax, int F, void* stream);

/* SpecAugment masks (feature_processor.py:10-43) on the padded batch, in place: for utterance b the frames
 * [t_masks[b][k][0], t_masks[b][k][1]) and the bins [f_masks[b][k][0], f_masks[b][k][1]) become `value`
 * (SPEC_MASK = 0); only the utterance's own nframes[b] frames are touched.  The (start, end) pairs are drawn on
 * the host in the reference's order (openeat_amd/augment.py), which makes the result bit-identical for a given seed. */
int oe_spec_augment(float* x, const int* nframes, int B, int Tmax, int F, const int* t_masks, int nt, const int* f_masks,
                    int nf, float value, void* stream);
/* Spec-substitute (feature_processor.py:45-64): subs (B, ns, 3) = (start, end, pos); rows [start, end) are replaced
 * by rows [start - pos, end - pos), one substitution after the other; end - start <= max_rows. */
int oe_spec_substitute(float* x, int B, int Tmax, int F, const int* subs, int ns, int max_rows, void* stream);
/* Feature dither (dataset.py:197-201): x += (u - 0.5) * a, u ~ U[0,1) from Philox(seed, element); only each utterance's
 * own nframes[b] frames.  Distribution parity with the reference (which uses numpy's global generator), not bit parity. */
int oe_feature_dither(float* x, const int* nframes, int B, int Tmax, int F, float a, unsigned long long seed, void* stream);

/* Speed perturbation of a padded waveform batch (audio_processor.py:20-35: sox `speed s` + `rate sr`): utterance b is
 * read speed[b] times faster and resampled back to the same rate, out[b, i] = x_b(i * speed[b]) through a Hann-windowed
 * sinc (cutoff 0.95 * min(1, 1/s), 16 zero crossings each side, unit DC gain); speed 1 copies.  wav (B, ld_in) with
 * n_in[b] valid samples, out (B, ld_out) with n_out[b] valid samples (the host sets n_out[b] = floor(n_in[b] / speed[b]
 * + 0.5)), samples past n_out[b] up to Nmax_out are zeroed.  sox itself is outside the reference tree: distribution
 * parity, checked against a float64 restatement and scipy's polyphase resampler. */
int oe_speed_perturb(const float* wav, long ld_in, const int* n_in, const float* speed, int B, int Nmax_out, float* out,
                     long ld_out, const int* n_out, void* stream);

/* A back-off n-gram (ARPA) language model as the kernels read it (built by openeat_amd/models/ngram_lm.py, which states the
 * layout once more):
 *   unigrams (n_words, 2) f32 = (log10 p, back-off) by word id - every word is listed, <unk> included;
 *   table (capacity) slots of 16 bytes {u64 key, f32 log10 p, f32 back-off}, capacity a power of two >= twice the number of
 *     n-grams of order >= 2, open addressing with linear probing from murmur3_fmix64(key) & (capacity-1), empty key = ~0.
 *     An n-gram's entry number is its word id (order 1) or n_words + its slot; its key is
 *     (entry number of its first k-1 words) << 32 | id of its k-th word.  The key is the n-gram: lookups are exact.
 *     max_probe = the longest displacement of any stored key; a lookup reads at most max_probe + 1 slots.
 *   order 1..5; n_words + capacity < 2^31; bos_word / eos_word / unk_word the word ids of <s>, </s>, <unk>.
 *   tok2word (V) i32: token id -> word id (the <unk> id for tokens the model does not list); a token id outside 0..V-1 and a
 *     word id outside 0..n_words-1 count as <unk>.
 * The struct is host memory, read during the call only; the three pointers are device pointers. */
typedef struct oe_ngram_model {
    const float* unigrams;
    const void* table;
    const int* tok2word;
    long capacity;
    int n_words, max_probe, order, bos_word, eos_word, unk_word, V;
} oe_ngram_model;

/* Back-off n-gram (ARPA) language-model score of R hypotheses on the device, one wavefront per hypothesis
 * (asr_model.py:515-516: `lm.score(' '.join(content), bos=True, eos=True)` with kenlm, once per hypothesis on the host).
 * Total log10 probability, the ARPA back-off definition: with w the word ids of [<s> if bos] tok2word[tokens[r, :len]]
 * [</s> if eos] and h the up to order-1 words before position i (never reaching before the first word),
 *   p(w_i | h) = logp(h w_i) if that n-gram is listed, else backoff(h) + p(w_i | h without its first word),
 *   backoff(h) = 0 when h is not listed; <s> is context only and never scored.
 * model: an oe_ngram_model.  tokens (R, ld) i32, lens (R) i32: lens[r] < 0 = the slot does not exist (as out_len of
 * oe_ctc_prefix_beam); what lies behind lens[r] is never read.
 * Outputs: score (R) f64, -inf for a missing slot;  optional tok_logp (R, ld+1) f64 and tok_order (R, ld+1) i32: the term
 * and the matched n-gram length of token j at [r, j], of </s> at [r, len] when eos; entries behind that, and the whole
 * row of a missing slot, are left untouched.
 * One launch, no workspace, no atomics; float64 sums in a fixed order (bit-reproducible); capturable. */
int oe_ngram_score(const oe_ngram_model* model, const int* tokens, long ld, const int* lens, int R, int bos, int eos,
                   double* score, double* tok_logp, int* tok_order, void* stream);

/* The n-gram LM term of C candidate next tokens of each of R growing hypotheses: the conditional log10 p(w | hypothesis) a
 * search step mixes into its pruning key, where oe_ngram_score scores finished sequences.
 * Rows: row r is the hypothesis tokens[r, :lens[r]] (tokens (R, ld) i32, the tokens after <sos>; lens (R) i32);
 * lens[r] < 0 = the slot does not exist, lens[r] above ld is clamped to ld; what lies behind the length is never read.
 * Candidates: cand (R, C) i32, out[r, j] is for token cand[r, j];  cand == NULL = every token: C must equal model->V and
 * out[r, j] is for token j.  eos_tok: the token id whose word is </s> (-1: no token is).
 * The value: out[r, j] is the term oe_ngram_score would write to tok_logp[r, len] had the candidate been appended to the
 * hypothesis with bos = 1 - for the eos_tok candidate its </s> term, with eos = 1.  The same ARPA back-off definition: every
 * other token maps to its word as in oe_ngram_score (the blank, ids outside 0..V-1 and unmapped tokens count as <unk> and
 * get a finite value), the context is the last order-1 words of <s> + hypothesis, the back-offs of the longer listed
 * contexts are added in float64, longest first, the log10 p last - so the result is bit-identical to oe_ngram_score's
 * tok_logp and to NgramLM.full_scores on the host.  A missing slot: all C entries of its row are -inf.
 * out (R, C) f64.  An entry is the same bits whether its token is reached through cand or through the full-vocabulary
 * form, and for any grid shape.
 * Refused before any launch (oe_last_error): a null pointer other than cand, C < 1, cand == NULL with C != V, eos_tok
 * outside -1..V-1, ld < 0, and what every oe_ngram_model entry point refuses.
 * One launch, no workspace, no atomics, no allocation, no host read: capturable. */
int oe_ngram_next(const oe_ngram_model* model, const int* tokens, long ld, const int* lens, int R, const int* cand, int C,
                  int eos_tok, double* out, void* stream);

/* A context graph (the hotwords of the biased search below) as the kernel reads it - an Aho-Corasick automaton built by
 * openeat_amd/utils/context_graph.py, which states the layout once more.  States are trie nodes, the root is 0,
 * n_states <= 2^20:
 *   edges (capacity) slots of 16 bytes {u64 key, i32 next state, i32 0}: the TRIE edges only, in the table format of
 *     oe_ngram_model (open addressing, linear probing from murmur3_fmix64(key) & (capacity-1), empty key = ~0, capacity a
 *     power of two, max_probe the longest displacement), key = state << 32 | token.  A missing edge follows fail and
 *     tries again - depth falls with every step, so at most 32 steps and 33 probes; from the root a missing edge stays there.
 *   fail (n_states) i32: the longest proper suffix of the state that is a trie node.
 *   out (n_states, 2) 32-bit words = (f32 score, i32 link): the score of the phrase that ends exactly at the state (0.0
 *     if none does) and the nearest state on its fail chain at which a phrase ends (0: none).  The phrases that end at a
 *     position are kept as this LIST, longest first, and added one by one - a pre-summed value would not reproduce the
 *     float64 sum of hits(p) below.
 *   pend (n_states) i32: the depth of the first state on the chain s, fail[s], .. that has children, which is k(p).
 *   c: the per-token partial credit, finite and >= 0.
 * The struct is host memory, read during the call only; the four pointers are device pointers. */
typedef struct oe_context_graph {
    const void* edges;
    const int* fail;
    const void* out;
    const int* pend;
    long capacity;
    int max_probe, n_states;
    float c;
} oe_context_graph;

/* The hotword bias of C candidate next tokens of each of R growing hypotheses: what a search step that extends hypotheses
 * token by token adds to its pruning key - the counterpart of oe_ngram_next for an oe_context_graph.  hits(p), k(p) and
 * bias(p) are those of the biased prefix search, stated under oe_ctc_prefix_beam below; step(s, token) is the automaton's
 * transition as oe_context_graph describes it (the edge, on a miss fail and again).
 * Rows: row r is a hypothesis g that sits in automaton state state[r] ((R) i32; the root, 0, for the empty one) with
 * hits[r] = hits(g) ((R) f64).  A state[r] outside 0..n_states-1, negative ones included = the slot does not exist: its whole
 * row is out_state = -1, out_hits = out_bias = -inf.
 * Candidates: cand (R, C) i32, entry [r, j] is for token cand[r, j];  cand == NULL = every token: entry [r, j] is for token j
 * and C is the vocabulary size.  A token no edge carries - the blank, a negative id, an id beyond the vocabulary - is an
 * ordinary mismatch: the walk follows fail to wherever it ends; the key is built from the unsigned token.
 * A candidate other than eos_tok:  s' = step(state[r], token);  h' = hits[r] + the scores of the phrases that end at s',
 *   added one by one in float64 in the list order s', link[s'], .. (longest first);
 *   out_state = s', out_hits = h' = hits(g . token), out_bias = h' + (double)c * pend[s'] = bias(g . token) during the search.
 * The eos_tok candidate (-1: no token is): it is not walked - the hypothesis ends, so the pending credit is dropped as
 *   `final` drops it:  out_state = state[r], out_hits = hits[r], out_bias = hits[r].
 * out_state (R, C) i32 and out_hits (R, C) f64 may both be NULL and are then not written (a pre-selection over the whole
 * vocabulary needs out_bias only); one without the other is refused.  out_bias (R, C) f64.
 * An entry is the same bits whether its token is reached through cand or through the full-vocabulary form, and for any grid
 * shape; out_hits and out_bias are bit for bit ContextGraph.bias of the extended prefix on the host (final = True and
 * final = False), for the eos_tok candidate out_bias is that of the un-extended prefix with final = True.
 * Refused before any launch (oe_last_error): a null pointer other than cand, out_state or out_hits (the graph's among them),
 * R < 0, C < 1, eos_tok < -1, and what oe_ctc_prefix_beam refuses about an oe_context_graph: n_states outside 1..2^20, a
 * capacity that is no power of two >= 2, a bad max_probe, a non-finite or negative c.  R == 0 returns 0 without a launch.
 * Every index read from a table is checked against n_states.
 * One launch, no workspace, no atomics, no allocation, no host read: capturable. */
int oe_context_next(const oe_context_graph* ctx, const int* state, const double* hits, int R, const int* cand, int C,
                    int eos_tok, int* out_state, double* out_hits, double* out_bias, void* stream);

/* CTC prefix beam search on the device, one wavefront per utterance (asr_model.py:359-396; the host functions below are
 * the same algorithm on the CPU and serve as its checker): plain, with n-gram LM shallow fusion (lm != NULL), with hotword
 * biasing (ctx != NULL), or with both.  One entry point, one argument struct, four instantiations of one kernel:
 *   lm NULL, ctx NULL: the plain search;  lm set, ctx NULL: the LM-fused search;
 *   lm NULL, ctx set:  the biased search without an LM;  lm set, ctx set: the biased search with the LM.
 *
 * The plain search.  topk_logp (B, Tmax, beam) f32 and topk_idx (B, Tmax, beam) i64 as oe_topk_rows writes them; lens (B)
 * i32 valid frames per utterance or NULL; beam <= 16.  workspace: oe_ctc_prefix_beam_workspace_bytes(B, Tmax, beam) bytes of
 * device memory whose LAST 4-byte word the caller zeroes and reads back after the stream has drained (non-zero: a prefix
 * exceeded max_len); the same for every variant.  Outputs, device memory: out_prefix (B, beam, max_len) i32, out_len (B, beam)
 * i32 (-1: fewer than `beam` prefixes exist), out_score (B, beam) f64 = log_add(pb, pnb), in the search's own order (no
 * re-sort).  out_ctc, out_lm and out_bias are neither required nor written; eos and final are not read.  lm_weight and
 * length_bonus must be 0: the plain search has no such terms, and a non-zero one is reported, not ignored.
 *
 * With n-gram LM shallow fusion (lm != NULL).  These are the semantics every layer refers to.  It is the algorithm of the
 * plain search (asr_model.py:359-396) with one change, the key that orders next_hyps before the cut to `beam`:
 *   total(p) = log_add(pb, pnb) + lm_weight * LM(p) + length_bonus * len(p)
 *   LM(p)    = sum over i < len(p), left to right in float64, of log10 p(word(p_i) | h_i)
 * LM terms: p(w | h) is the ARPA back-off definition exactly as oe_ngram_score states it - h the up to order-1 previous
 *   words, starting from <s>, which is context only and never scored; token -> word through tok2word; out-of-range ids count
 *   as <unk>.  So LM(p) is oe_ngram_score(p, bos=1, eos=0) up to summation order.
 * Units: log10, mixed in unconverted, as the reference and the rescoring do with kenlm's numbers.
 * Per-frame updates: the pb / pnb updates are unchanged, the same arithmetic in the same visiting order; the CTC numbers
 *   are the same bits as the plain search's.
 * Sort order: stable and descending by total, so ties keep insertion order (the first-touch stamp).
 * LM(p) depends on the prefix only: the two routes that merge into one prefix carry the same value and the same LM state.
 * End of the utterance: if eos, every surviving prefix gets LM += log10 p(</s> | its context); the <= beam survivors are
 *   stably re-sorted by total.  An utterance of zero frames yields the one empty prefix, with LM = p(</s> | <s>) when eos.
 * Outputs per (b, slot), device memory: out_prefix (B, beam, max_len) i32 and out_len (B, beam) i32 with -1 for a missing
 *   slot; out_score = total, out_ctc = log_add(pb, pnb), out_lm = LM including the </s> term, each (B, beam) f64 and -inf
 *   for a missing slot; the status word of the workspace as for the plain search.
 * Identity with zero weights: with lm_weight == 0 and length_bonus == 0 the n-best lists and their order are those of
 *   the plain search, and out_ctc equals its out_score bit for bit.
 * topk_logp / topk_idx / lens / beam (<= 16) / max_len / workspace as for the plain search; lm an oe_ngram_model
 * (order <= 5); lm_weight and length_bonus finite.  Anything else, and a null pointer other than lens, is reported through
 * oe_last_error before any launch.  One launch, no atomics other than the status word, no allocation, no host read: capturable.
 *
 * With hotword (contextual) biasing (ctx != NULL), with or without the n-gram LM.  These are the semantics every layer
 * refers to.
 * A context graph is a set of distinct phrases q, each a sequence of 1..32 token ids in 1..V-1 (never the blank) with a
 * float32 score s(q), and one float32 per-token partial credit c >= 0; by default s(q) = c * len(q) in float32.  For a
 * token prefix p:
 *   hits(p) = the sum of s(q) over every occurrence of every phrase in p, an occurrence being a pair (i, q) with
 *             p[i-len(q):i] == q, 1 <= i <= len(p); overlapping and nested occurrences all count.  The float32 values are
 *             added in float64 in order of increasing i, within one i the longest phrase first.
 *   k(p)    = the largest k <= len(p) such that the last k tokens of p are a PROPER prefix of some phrase (strictly
 *             shorter than it); 0 if there is none.
 *   bias(p) = hits(p) + (double)c * k(p) during the search; at the end of the utterance, with `final` set, the pending
 *             credit is dropped: bias(p) = hits(p).
 * Partial credit keeps a half-spoken hotword in the beam; it is taken back when the phrase fails and at the end of the audio.
 * The search is the LM-fused one with one more summand, products and sums each rounded on their own:
 *   total(p) = ((log_add(pb, pnb) + lm_weight * LM(p)) + length_bonus * len(p)) + bias(p)
 *   without an LM (lm == NULL):  total(p) = (log_add(pb, pnb) + length_bonus * len(p)) + bias(p).
 * The pb / pnb updates, the visiting order, the first-touch stamps and the stable descending sort are unchanged.  bias(p)
 * depends on the prefix only: two routes that merge into one prefix carry the same value and the same automaton state.
 * End of the utterance: (1) the </s> LM term if an LM is given and eos; (2) the pending credit dropped if final; (3) the
 * survivors stably re-sorted by total.  An utterance of zero frames yields the one empty prefix with bias 0.
 * Identities: with an empty graph, and with one whose scores and c are all zero, the n-best lists, their order, out_ctc,
 *   out_lm and out_score are bit for bit those of the LM-fused search with the same LM arguments; without an LM and with
 *   length_bonus == 0 the lists and out_ctc are bit for bit those of the plain search.
 * Arguments: those of the LM-fused search, ctx (an oe_context_graph), final, out_bias (B, beam) f64 = bias as it entered
 * out_score, -inf for a missing slot.  lm == NULL means no LM: out_lm may then be NULL, lm_weight and eos are ignored and
 * out_lm is not written.  Checked before any launch and reported through oe_last_error: null pointers (args, the model's and
 * the graph's among them), beam 1..16, non-finite weights or c, c < 0, the model checks of the LM-fused search, n_states
 * 1..2^20, a power-of-two capacity of the graph, its max_probe.  One launch, no atomics other than the status word, no
 * allocation, no host read: capturable.
 *
 * The structs are host memory, read during the call only: the launch copies what the kernel takes. */
typedef struct oe_prefix_beam_args {
    const float* topk_logp;
    const long long* topk_idx;
    const int* lens;              /* NULL: every utterance has Tmax frames */
    int B, Tmax, beam, max_len;
    const oe_ngram_model* lm;     /* NULL: no LM */
    const oe_context_graph* ctx;  /* NULL: no graph */
    double lm_weight, length_bonus;
    int eos, final;               /* eos: read only with an LM; final: read only with a graph */
    void* workspace;
    int* out_prefix;
    int* out_len;
    double* out_score;
    double* out_ctc;              /* with an LM or a graph */
    double* out_lm;               /* with an LM */
    double* out_bias;             /* with a graph */
} oe_prefix_beam_args;
size_t oe_ctc_prefix_beam_workspace_bytes(int B, int Tmax, int beam);
int oe_ctc_prefix_beam(const oe_prefix_beam_args* args, void* stream);
/* The same search, resumable: it takes the frames of an utterance chunk by chunk and carries everything it knows in a device
 * state, for recordings whose frames arrive window by window and whose back-pointers would not fit as a whole.  The four
 * variants are those of oe_ctc_prefix_beam (lm / ctx of `search`), from the same kernel source.
 *
 * search: the oe_prefix_beam_args of THIS chunk - topk_logp / topk_idx (B, Tmax, beam), lens (B) the frames of this chunk
 *   (0 allowed; NULL: Tmax), beam, max_len, lm, ctx, the weights, eos, final, the out_* and a workspace of
 *   oe_ctc_prefix_beam_workspace_bytes(B, Tmax, beam) bytes: the back-pointers are those of the chunk, never of the recording.
 *   Its last word is the status word, zeroed and read by the caller as for the one-shot search.
 * The state, oe_ctc_prefix_beam_state_bytes(B, beam, max_len) bytes of device memory (the size is the same for every
 *   variant), is opaque.  Per utterance it carries what the frame loop keeps between two frames - the number of live
 *   prefixes, the number of frames consumed so far, per slot key, pb, pnb, len, last, with an LM lm, ent[], bo[], with a graph
 *   hits, the automaton state, pend - and every slot's tail: the tokens and emission frames behind the stable prefix.  Its
 *   header records B, beam, max_len and the variant (LM / graph); the kernel checks it against the call and on a mismatch
 *   writes 2 into the status word and touches no output, no state and no stable buffer.  The LM entry numbers and the
 *   automaton states are indices into the tables of the model and the graph: a state is valid only with the SAME model and the
 *   SAME graph (and weights) it was made with, which nothing checks.
 * A chunk resumes the frame loop at state_in (NULL: the search starts here, with the empty prefix) and runs lens[b] frames.
 *   Without `last` it saves the state to state_out and does nothing else to the scores.  lens[b] == 0 carries utterance b
 *   through untouched: so a batch of recordings of different lengths ends together in one `last` call.  state_out must not be
 *   state_in (the tails are read from one while the other is written): the caller keeps two and swaps them.
 * With `last` the end-of-utterance steps run exactly as in the one-shot search: the </s> term, the pending hotword credit
 *   dropped if final, the stable re-sort.  For ANY sequence of chunks whose frames concatenate to an utterance - chunks of one
 *   frame, of zero frames, a single chunk with state_in == NULL and last - out_prefix (its used part) / out_len / out_score /
 *   out_ctc / out_lm / out_bias are bit for bit what oe_ctc_prefix_beam writes for that utterance.  state_out may be NULL
 *   with last; the stable buffers are then left as they are.
 * Stable prefix.  After every chunk with a state_out, stable_len[b] is the length of the longest common prefix of utterance
 *   b's live prefixes.  Every later prefix extends a live one, so these tokens never change and stable_len never shrinks.
 *   Newly stable tokens and their frames are appended to stable_prefix / stable_frame (B, max_len), which the caller owns
 *   and only the kernel appends to; the caller zeroes stable_len (B) before the first chunk.  The tails of the state shrink
 *   by what was committed, so a chunk's work is proportional to its frames plus the tail lengths, not to the transcript so
 *   far (an emitting chunk also writes the n-best rows in full).
 * Emission frame.  The emission frame of a token is the global frame index t, counted over all chunks, at which the prefix
 *   ending in that token was created as a new entry on the slot's back-pointer chain (the frame whose record carries the
 *   token).  A prefix that stays, or that an extension lands on, keeps its frames; one that dropped out of the beam and is
 *   created again has the later frame.  Frames are strictly increasing along a prefix.  The chains of two live prefixes can
 *   disagree about the frame of a shared token (one went through the prefix before it dropped out, the other through its
 *   re-creation): the stable prefix commits the earliest, and out_frame reports committed tokens with the committed frame.
 * emit without last: the n-best is written in the search's own order with the running totals as the pruning key sees them -
 *   no </s> term, the pending credit kept; missing slots -1 / -inf as in the one-shot search; out_prefix is the stable prefix
 *   followed by the tail, out_frame (B, beam, max_len) or NULL the emission frame of each of its tokens.  With last the outputs
 *   are always written.  A prefix longer than max_len sets the status word to 1, as in the one-shot search; the state is then
 *   of no further use.
 * Checked before any launch and reported through oe_last_error: a null chunk or search, everything oe_ctc_prefix_beam
 *   checks, state_out == NULL without last, state_in == state_out, a null stable_prefix / stable_frame / stable_len.  One
 *   launch, no atomics other than the status word, no allocation, no host read: capturable. */
typedef struct oe_prefix_beam_chunk {
    const oe_prefix_beam_args* search;
    const void* state_in;         /* NULL: the search starts here */
    void* state_out;              /* NULL allowed only with last; never state_in */
    int last;                     /* the audio of every utterance ends with this chunk */
    int emit;                     /* write the n-best outputs for this chunk (always done when last) */
    int* stable_prefix;           /* (B, max_len) */
    int* stable_frame;            /* (B, max_len) */
    int* stable_len;              /* (B) in/out */
    int* out_frame;               /* (B, beam, max_len) or NULL */
} oe_prefix_beam_chunk;
size_t oe_ctc_prefix_beam_state_bytes(int B, int beam, int max_len);
int oe_ctc_prefix_beam_chunk(const oe_prefix_beam_chunk* chunk, void* stream);
/* CTC prefix beam search, HOST code (all pointers are host pointers): the per-frame recursion of
 * asr_model.py:359-396 on the top-`beam` (log-prob, token) pairs of every frame (computed on the
 * device).  Doubles and insertion-ordered stable pruning as in the reference's Python, so the
 * n-best list and scores are identical.  out_prefix_host (beam, max_len) int32, out_len_host (beam)
 * (-1 = fewer than `beam` hypotheses), out_score_host (beam) = log_add(pb, pnb). */
int oe_ctc_prefix_beam_host(const float* topk_logp_host, const long long* topk_idx_host, int T, int beam,
                            int max_len, int* out_prefix_host, int* out_len_host, double* out_score_host);
/* The same for B utterances at once, spread over n_threads host threads (<= 0: all cores): inputs (B, Tmax, beam) with
 * lens[b] valid frames each; outputs (B, beam, max_len) / (B, beam) / (B, beam). */
int oe_ctc_prefix_beam_host_batch(const float* topk_logp_host, const long long* topk_idx_host, int B, int Tmax,
                                  const int* lens_host, int beam, int max_len, int* out_prefix_host, int* out_len_host,
                                  double* out_score_host, int n_threads);

/* Batched edit distance on the device, one wavefront per pair: the counts behind the reference's error-rate table
 * (tools/compute-wer.py, Calculator.calculate) and optionally the alignment.  These are the semantics every layer refers to.
 * For a reference r[0..n) and a hypothesis h[0..m) of token ids, costs cor 0, sub 1, del 1, ins 1:
 *   D[i][0] = i (all deletions), D[0][j] = j (all insertions);
 *   for i, j >= 1 the predecessor is chosen in the order deletion (i-1, j), insertion (i, j-1), diagonal (i-1, j-1)
 *   (cor if r[i-1] == h[j-1], else sub); a later candidate replaces the best only if it is strictly smaller;
 *   the alignment is the chain of chosen predecessors from (n, m) back to (0, 0); cor, sub, del, ins count its moves, so
 *   cor + sub + del = n and the error rate is (sub + del + ins) / n.
 * Pair p compares hyp row p (hyp_lens[p] tokens) with ref row p / group (ref_lens[p / group] tokens): group = 1 is
 * one-to-one, group = beam an n-best list against its utterance.  ref (P / group, ref_ld), hyp (P, hyp_ld) i32; what lies at
 * or behind a row's length never reaches a result.  hyp_lens[p] < 0 = the slot does not exist (as out_len of
 * oe_ctc_prefix_beam): counts (-1, -1, -1, -1), every ref_to_hyp entry -1.
 *   out: counts (P, 4) i32 = cor, sub, del, ins;  ref_to_hyp (P, Nmax) i32 or NULL: the hypothesis position aligned with
 *        reference token i (cor or sub), -1 if it is deleted, -1 for i >= n; inserted hypothesis tokens are those no entry names.
 *   0 <= Nmax, Mmax <= 1023; group >= 1, P % group == 0, ref_ld >= Nmax, hyp_ld >= Mmax - anything else, and a null required
 *   pointer, is reported through oe_last_error before any launch.  The lengths live on the device: one above its maximum is
 *   clamped to it by the kernel (a negative ref length counts as 0).
 *   workspace: oe_edit_distance_workspace_bytes(P, Nmax, Mmax) bytes, 4-byte aligned; 0 (NULL allowed) when ref_to_hyp is NULL
 *   or the 2-bit back-pointers fit LDS (Nmax * ceil(Mmax / 16) * 4 <= 48 KiB).
 * With ref_to_hyp == NULL the counts are carried forward along the chosen predecessors and no workspace is touched.
 * One launch; no atomics, no allocation, no synchronisation, no host-side state: capturable. */
size_t oe_edit_distance_workspace_bytes(int P, int Nmax, int Mmax);
int oe_edit_distance(const int* ref, long ref_ld, const int* ref_lens, int group, const int* hyp, long hyp_ld,
                     const int* hyp_lens, int P, int Nmax, int Mmax, int* counts, int* ref_to_hyp, void* workspace,
                     void* stream);

/* CTC prefix scores for the joint CTC/attention one-pass beam search (Watanabe et al. 2017, Hori et al. 2017): the attention
 * decoder proposes tokens and the CTC prefix score of every proposal enters the pruning key.  These are the semantics every
 * layer refers to (ops.ctc_prefix_score, utils/joint_search.py, ASRModel.ctc_attention_beam_search; the yardstick is
 * tests/ctc_prefix_score_ref.py).
 *
 * y[t, k] are the CTC log-probabilities of one utterance, t = 0..T-1, T its valid frame count; column `blank` is the blank.
 * A hypothesis is a token sequence g (the tokens after <sos>).  Its state is r[t, 0] (non-blank) and r[t, 1] (blank): the
 * log-probability of all alignments of frames 0..t that collapse to exactly g and end in a non-blank resp. a blank.
 *   The empty hypothesis: r[t, 0] = -inf, r[t, 1] = y[0, blank] + .. + y[t, blank], added left to right.
 *   Extension h = g . c with c neither blank nor <eos>:
 *     n[0, 0] = y[0, c] if g is empty else -inf;  n[0, 1] = -inf;  psi = n[0, 0]
 *     for t = 1..T-1:
 *       phi     = r[t-1, 1]                        if c == the last token of g
 *                 log_add(r[t-1, 0], r[t-1, 1])    otherwise
 *       n[t, 0] = log_add(n[t-1, 0], phi) + y[t, c]
 *       n[t, 1] = log_add(n[t-1, 0], n[t-1, 1]) + y[t, blank]
 *       psi     = log_add(psi, phi + y[t, c])
 *   psi(h) is the log-probability that the utterance's label sequence starts with h; n is h's state.
 *   c blank or outside 0..V-1: psi = -inf (this is tested first).  c == <eos>: psi = log_add(r[T-1, 0], r[T-1, 1]), the full
 *   CTC likelihood of g.  T == 0: <eos> after the empty hypothesis scores 0, everything else -inf.  In none of these cases
 *   is a state produced: the candidate's cand_state entries are not written.
 *   log_add(a, b) = max + log(exp(a - max) + exp(b - max)); with both arguments -inf it is -inf, never NaN.  All arithmetic
 *   is float64, as in the prefix-beam kernels.
 *
 * logp (B, Tmax, ldv) f32 with ldv >= V; lens (B) i32 valid frames (clamped to 0..Tmax by the kernel) or NULL = Tmax.  There
 * are R = B * group rows; row r belongs to utterance r / group.
 * oe_ctc_prefix_score_init writes the empty hypothesis' state of every row into state (R, Tmax, 2) f64.
 * oe_ctc_prefix_score: state_in (R, Tmax, 2) f64 the hypotheses' states; hyp_len (R) i32 their token counts (0: the empty
 * one), < 0 = the slot does not exist (as out_len of oe_ctc_prefix_beam): all its psi are -inf and its cand_state rows are
 * untouched; last_tok (R) i32, read where hyp_len > 0; cand (R, C) i32 candidate tokens, 1 <= C <= 64.
 *   out: psi (R, C) f64;  cand_state (R, Tmax, C, 2) f64 or NULL: the state of hypothesis r extended by its candidate j at
 *        [r, t, j, :].  psi is bit-identical with and without cand_state.
 * Frames at or beyond an utterance's length are never read or written, in any buffer.
 * Null pointers (other than lens and cand_state), C outside 1..64, group < 1, ldv < V and a blank outside 0..V-1 are
 * reported through oe_last_error before any launch.  One wavefront per row, one lane per candidate; one launch, no workspace,
 * no atomics, no allocation, no synchronisation, no host-side state: capturable. */
int oe_ctc_prefix_score_init(const float* logp, const int* lens, int B, int Tmax, int V, long ldv, int group, int blank,
                             double* state, void* stream);
int oe_ctc_prefix_score(const float* logp, const int* lens, int B, int Tmax, int V, long ldv, int group, const double* state_in,
                        const int* hyp_len, const int* last_tok, const int* cand, int C, int blank, int eos, double* psi,
                        double* cand_state, void* stream);

/* Differentiable n-best CTC scoring: the exact CTC log-likelihood of each of `group` hypotheses of an utterance and the
 * gradient of a weighted sum of them with respect to the utterance's logits - the device half of minimum word error rate
 * training over n-best lists (Prabhavalkar et al. 2018; utils/mwer.py, ASRModel.forward_mwer).  These are the semantics every
 * layer refers to (ops.ctc_nbest_logp; the yardstick is tests/ctc_nbest_ref.py).
 *
 * There are R = B * group rows; row r belongs to utterance r / group; blank = 0.  logits (B, T, ldv >= V) f32 and hlens (B)
 * i32 as oe_ctc_loss_fused (hlens is clamped to 0..T by the kernel).  hyps (R, hyp_ld >= Lmax) i32, hyp_lens (R) i32; a
 * negative length = the slot does not exist (as out_len of oe_ctc_prefix_beam).  1 <= group <= 64, 0 <= Lmax <= 255.
 *
 * oe_ctc_nbest_score: logp (R) f32.  logp[r] is the natural log of the sum, over all alignments of the utterance's
 *   Tb = hlens[b] frames that collapse to hypothesis r, of the product of the frames' softmax probabilities - the trellis of the
 *   loss: blank, y1, blank, .., blank.  A row is INFEASIBLE if the slot does not exist, hyp_lens[r] > Lmax (a hypothesis is
 *   never truncated), Tb == 0, Tb < length + the number of adjacent equal tokens, or a token within the length lies outside
 *   1..V-1 (such a token is never used as an index).  An infeasible row has logp = -inf exactly and contributes nothing to
 *   dlogits.  An empty hypothesis with Tb > 0 is feasible: every frame blank.  logp[r] depends on its own row only: permuting
 *   the slots of a group permutes the bits of logp.  What lies at or behind a row's length never reaches a result.
 *   saved: NULL, or oe_ctc_nbest_saved_bytes(B,T,group,Lmax) bytes, 16-byte aligned, opaque: what the forward keeps so that
 *   oe_ctc_nbest_grad need not run the recursions again.  logp is bit-identical with and without it.
 *   workspace: oe_ctc_nbest_workspace_bytes(B,T,group,Lmax) bytes, 16-byte aligned.
 * oe_ctc_nbest_grad: the same logits, hlens, hyps, hyp_lens, group, Lmax as the score call that filled `saved`, and its logp;
 *   g (R) f32 the weights.  For t < Tb and v < V
 *     dlogits[b,t,v] = sum over the feasible rows r of b of  g[r] * (occ_r[t,v] - softmax(logits[b,t,:])[v]),
 *   occ_r[t,v] the posterior probability that hypothesis r's alignment emits class v at frame t: the gradient of
 *   sum_r g[r] * logp[r] with respect to the raw logits.  Rows t >= Tb are written as exact zeros; columns >= V are not
 *   written.  g of an infeasible row is not read into any result (it may be NaN).  dlogits (B, T, ldv) may not alias logits.
 *   workspace: not used by this call; NULL is allowed.
 * Both calls: no float atomics, every sum in a fixed order (bit-identical from run to run); no allocation, no
 * synchronisation, no host-side state: capturable.  Null required pointers, group or Lmax outside their ranges, ldv < V,
 * hyp_ld < Lmax and dlogits == logits are reported through oe_last_error before any launch.
 * Passes: score = one wave per frame reads the logits once (row statistics, log-probabilities at the hypotheses' states), then
 * one block per row runs alpha and - with `saved` - beta and the occupancies; grad = one workgroup per dlogits row. */
size_t oe_ctc_nbest_workspace_bytes(int B, int T, int group, int Lmax);
size_t oe_ctc_nbest_saved_bytes(int B, int T, int group, int Lmax);
int oe_ctc_nbest_score(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* hyps, long hyp_ld,
                       const int* hyp_lens, int group, int Lmax, float* logp, void* saved, void* workspace, void* stream);
int oe_ctc_nbest_grad(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* hyps, long hyp_ld,
                      const int* hyp_lens, int group, int Lmax, const float* logp, const float* g, const void* saved,
                      float* dlogits, void* workspace, void* stream);

/* Transducer (RNN-T) loss on device: the log-likelihood of a label sequence under the transducer lattice (Graves 2012, the
 * interface of warp-transducer) and its gradient with respect to the raw joint logits.  No counterpart in the reference, which
 * has no transducer.  These are the semantics every layer refers to (ops.rnnt_loss; the yardstick is tests/rnnt_ref.py).
 *   logits (B, T, Umax+1, ldv >= V) f32, raw.  hlens (B) i32 frames, ulens (B) i32 labels, targets (B, Umax) i32 (NULL allowed
 *   when Umax = 0), all on the device.  For utterance b: Tb = hlens[b] held to 0..T, Ub = ulens[b], y_1..y_Ub = targets[b,:Ub],
 *     lp(t,u,v) = logits[b,t,u,v] - logsumexp_v logits[b,t,u,:]
 *     alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lp(t-1,u,blank), alpha(t,u-1) + lp(t,u-1,y_u))
 *     logp[b] = alpha(Tb-1,Ub) + lp(Tb-1,Ub,blank)
 *     beta(Tb-1,Ub) = lp(Tb-1,Ub,blank);  beta(t,u) = logaddexp(beta(t+1,u) + lp(t,u,blank), beta(t,u+1) + lp(t,u,y_{u+1}))
 *   Tb = 0 gives logp[b] = -inf exactly and a zero gradient (the zero-infinity convention of oe_ctc_loss_fused).  What only the
 *   device can see is checked there, without a fault: ulens[b] outside 0..Umax, or a target within the length that is blank or
 *   outside 0..V-1 (it is never used as an index), makes the utterance INFEASIBLE: status[b] = 1, logp[b] = -inf, a zero
 *   gradient; status[b] = 0 otherwise.  status (B) i32 may be NULL.
 * oe_rnnt_loss: the row pass and the lattice pass; writes logp (B) f32 and leaves in `workspace` what oe_rnnt_grad needs.
 *   workspace: oe_rnnt_workspace_bytes(B,T,Umax) bytes, 16-byte aligned; with N = B*T*(Umax+1): the row log-sum-exp (4N,
 *   [b][t][u]), lp of the blank and of the next label (4N each, [b][u][t]), alpha and beta (8N each, [b][u][t]), logZ in the
 *   log2 domain (8B) and a status word per utterance (4B), each part rounded up to 16 bytes.
 * oe_rnnt_grad: the same logits, ldv, shape, hlens, targets, ulens, blank and workspace as the oe_rnnt_loss call before it, the
 *   logits unchanged since; g (B) f32.  At a node t < Tb, u <= Ub of a feasible utterance
 *     e_b = exp(alpha(t,u) + lp(t,u,blank)   + beta(t+1,u) - logp)   (beta(Tb,Ub) := 0; absent for t = Tb-1, u < Ub)
 *     e_y = exp(alpha(t,u) + lp(t,u,y_{u+1}) + beta(t,u+1) - logp)   (absent for u = Ub)
 *     dlogits[b,t,u,v] = g[b] * ([v = blank] e_b + [v = y_{u+1}] e_y - (e_b + e_y) * softmax(t,u)[v])
 *   the gradient of sum_b g[b] * logp[b].  The node's occupancy is the sum of its outgoing terms, never exp(alpha + beta - logp):
 *   at a confident node the cancellation against softmax ~ 1 then carries no drift of the recursions.  Every other node of the
 *   (B, T, Umax+1) grid is written as exact zeros; columns >= V are never written.  g of an infeasible utterance is not read into
 *   any result (it may be NaN).  dlogits (B, T, Umax+1, ldv) MAY be the logits buffer itself (the convention of
 *   oe_lsm_loss_fused): every element is read before it is written, by the same lane.
 * Numbers: the row pass sums exp in float32 and keeps lp = (x - max) - log(sum); alpha and beta are float64 in the log2 domain
 *   with the finite "log 0" of the CTC kernels, exp / log float32 on differences.  Against the float64 restatement: logp rtol
 *   1e-4 / atol 1e-3, gradient rtol 2e-3 / atol 2e-5 * |g[b]|, the tolerances of oe_ctc_loss_fused; the measured fractions are
 *   in DESIGN.md.
 * Limits: 1 <= B, 1 <= T <= OE_RNNT_MAX_T, 0 <= Umax <= OE_RNNT_MAX_U, 2 <= V, ldv >= V, 0 <= blank < V, B*T*(Umax+1) < 2^31.
 *   Anything else, a NULL required pointer (logits, hlens, ulens, targets when Umax > 0, logp / g, dlogits, workspace) and a
 *   workspace not 16-byte aligned are reported through oe_last_error before any launch, with the outputs untouched.
 *   oe_rnnt_workspace_bytes returns 0 outside the limits.
 * Launches: row pass, one wave per node inside the lattice (nodes outside are not read); lattice pass, one workgroup of two
 *   waves per utterance, alpha and beta side by side, a lane per label position (1, 2 or 4 positions per lane), a step per
 *   anti-diagonal, the label predecessor by one DPP shift, lp fetched a chunk of steps ahead; gradient pass, one wave per node.
 *   No float atomics, every sum in a fixed order: outputs are bit-identical from run to run.  No allocation, no host read, no
 *   host-side state: capturable. */
#define OE_RNNT_MAX_T 8192
#define OE_RNNT_MAX_U 255
typedef struct oe_rnnt_args {
    const float* logits; long ldv; int B, T, Umax, V;
    const int* hlens;
    const int* targets;   /* (B, Umax) */
    const int* ulens;
    int blank;
    float* logp;          /* (B) */
    int* status;          /* (B) or NULL */
    void* workspace;
} oe_rnnt_args;
typedef struct oe_rnnt_grad_args {
    const float* logits; long ldv; int B, T, Umax, V;
    const int* hlens;
    const int* targets;
    const int* ulens;
    int blank;
    const float* g;       /* (B) */
    float* dlogits;       /* (B, T, Umax+1, ldv); may be logits */
    void* workspace;      /* as oe_rnnt_loss left it */
} oe_rnnt_grad_args;
size_t oe_rnnt_workspace_bytes(int B, int T, int Umax);
int oe_rnnt_loss(const oe_rnnt_args* args, void* stream);
int oe_rnnt_grad(const oe_rnnt_grad_args* args, void* stream);

/* The joint network's broadcast: z[b,t,u,:] = act(e[b,t,:] + p[b,u,:]) for e (B, T, J) and p (B, U1, J), U1 = Umax + 1, act one
 * of the activation codes (0 none, 1 relu, 2 swish, 3 tanh, 4 hardtanh, 5 selu, 6 gelu).  No counterpart in the reference.
 *   hlens, ulens (B) i32 or NULL (NULL: every frame / every position).  A node is inside the lattice when t < hlens[b] and
 *   u <= ulens[b].  The forward writes EVERY node of z (B, T, U1, J): zeros outside the lattice, because the projection behind it
 *   reads them all.  The backward recomputes the pre-activation from e and p (nothing is stored):
 *     de[b,t,:] = sum over u of dz[b,t,u,:] * act'(e[b,t,:] + p[b,u,:])   one workgroup per (b,t), u ascending
 *     dp[b,u,:] = sum over t of dz[b,t,u,:] * act'(e[b,t,:] + p[b,u,:])   one workgroup per (b,u), t ascending
 *   over the nodes inside the lattice only; rows (b,t) and (b,u) with no such node are zeros.  The order of every sum is fixed:
 *   bit-identical from run to run.  Limits: 1 <= B, T, U1, J and B*T*U1 < 2^31; NULL e, p, z (dz, de, dp) and an unknown act are
 *   reported before any launch.  One launch each, no workspace, no atomics: capturable. */
typedef struct oe_joint_combine_args {
    const float* e; const float* p; int B, T, U1, J, act;
    const int* hlens; const int* ulens;
    float* z;
} oe_joint_combine_args;
typedef struct oe_joint_combine_bwd_args {
    const float* e; const float* p; int B, T, U1, J, act;
    const int* hlens; const int* ulens;
    const float* dz;
    float* de; float* dp;
} oe_joint_combine_bwd_args;
int oe_joint_combine_fwd(const oe_joint_combine_args* args, void* stream);
int oe_joint_combine_bwd(const oe_joint_combine_bwd_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENEAT_HIP_H */
