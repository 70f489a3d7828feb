// CTC head on device: softmax rows, alpha/beta recursion with wave shuffles,
// gradient w.r.t. the logits, and greedy search.
//
// Replaces  /root/reference/openeat/modules/ctc.py:38-45  (log_softmax ->
// torch.nn.CTCLoss(sum, zero_infinity) -> /B and its autograd) and
// /root/reference/openeat/models/asr_model.py:318-325 (greedy).
//
// Pass structure (HBM-bound; B*T*V*4 bytes = the logits):
//   k1 rows     : one wave per frame holds its row in registers: read logits ONCE, write
//                 softmax * scale ONCE (the dense part of the gradient, in place if asked),
//                 and emit lp[b,t,s] = log2-prob at the 2L+1 states
//   k2 alphabeta: one block per utterance, wave 0 runs alpha, wave 1 runs beta
//                 concurrently; neighbours s-1,s-2 come from lane shuffles; lp is
//                 prefetched a whole chunk of frames ahead (registers), so a step costs the
//                 shuffle + lse3 chain and not a global-memory round trip
//   k3 labels   : per frame, the <= 2L+1 classes that occur in the target get
//                 (softmax - sum_{s:l'_s=c} exp(alpha+beta-lp-ll)) * scale (states of one class are
//                 linked once per utterance by a third wave of k2); rows of infeasible
//                 utterances are zeroed (zero_infinity)
// Algorithmic bytes: 2*B*T*V*4 (+ 3 small state arrays), which is what k1 moves.
#include <stdlib.h>
#include <type_traits>
#include "oe_common.h"
#include "ctc_f64.h"
#include "../../include/openeat_hip.h"

#define NEG_INF (-INFINITY)
#define CTC_MAXQ 8          // states per lane in k1 / k3 (Sp <= 64 * 8)

// Store the float4 that starts at column e of a row of V columns: whole if it lies inside the row, else only its columns
// below V - the row padding (ldv > V) is never written.
__device__ __forceinline__ void ctc_store4(float* g, int e, int V, float4 o) {
    if (e + 3 < V) {
        *reinterpret_cast<float4*>(g + e) = o;
    } else {
        if (e < V) g[e] = o.x;
        if (e + 1 < V) g[e + 1] = o.y;
        if (e + 2 < V) g[e + 2] = o.z;
    }
}

// ------------------------------------------------------------------ k1 ------
// NV4 > 0: the row is NV4 float4 per lane (V <= 256 * NV4; rows 16-byte aligned and padded to a multiple of four floats);
// NV4 == 0: any V / alignment, the row is read twice (the second time from L2).
// dlogits is not __restrict__: it may alias logits (every load of a row is issued before its first store).
template <int NV4, bool WRITE>
__global__ __launch_bounds__(256) void ctc_rows_kernel(const float* logits, long ldv, long rows, int T, int V,
                                                        const int* __restrict__ hlens, const int* __restrict__ targets,
                                                        int Lmax, const int* __restrict__ tlens, int Sp, float scale,
                                                        const float* __restrict__ utt_weight, float* __restrict__ lp_out,
                                                        float* dlogits, int t0, int Tc) {
    // frames t0 .. t0 + Tc - 1 of every utterance (`rows` = B * Tc of them; the whole batch: t0 = 0, Tc = T)
    const int lane = threadIdx.x & 63;
    const long rloc = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rloc >= rows) return;
    const int b = (int)(rloc / Tc), t = t0 + (int)(rloc % Tc);
    const long row = (long)b * T + t;
    const float* p = logits + row * ldv;
    float* g = WRITE ? dlogits + row * ldv : nullptr;
    const int nv = (V + 3) >> 2;
    if (t >= hlens[b]) {                      // padded frame: exact zeros, no statistics
        if (WRITE) {
            if (NV4 > 0) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int i = lane; i < nv; i += 64) ctc_store4(g, 4 * i, V, z);
            } else {
                for (int i = lane; i < V; i += 64) g[i] = 0.f;
            }
        }
        return;
    }
    if (WRITE && utt_weight) scale *= utt_weight[b];
    const int L = min(tlens[b], Lmax);
    const int S = 2 * L + 1;
    // logits at the states' classes, loaded together with the row
    float lv[CTC_MAXQ];
#pragma unroll
    for (int q = 0; q < CTC_MAXQ; ++q) {
        const int st = lane + 64 * q;
        lv[q] = 0.f;
        if (st < S) lv[q] = p[(st & 1) ? targets[(long)b * Lmax + (st >> 1)] : 0];
    }
    float m, l2s;          // log-softmax in base 2 = (x - m) * log2(e) - log2(sum exp(x - m))
    if (NV4 > 0) {
        float4 v[NV4 > 0 ? NV4 : 1];
        const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int i = lane + 64 * j;
            v[j] = make_float4(NEG_INF, NEG_INF, NEG_INF, NEG_INF);
            if (i < nv) v[j] = p4[i];
        }
        m = NEG_INF;
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int e = (lane + 64 * j) * 4;        // columns past V (row padding) do not count
            if (e + 1 >= V) v[j].y = NEG_INF;
            if (e + 2 >= V) v[j].z = NEG_INF;
            if (e + 3 >= V) v[j].w = NEG_INF;
            m = fmaxf(m, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
        }
        m = wave_max(m);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            v[j].x = __expf(v[j].x - m); v[j].y = __expf(v[j].y - m);
            v[j].z = __expf(v[j].z - m); v[j].w = __expf(v[j].w - m);
            s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        }
        s = wave_sum(s);
        l2s = __builtin_amdgcn_logf(s);
        if (WRITE) {
            const float f = scale / s;
#pragma unroll
            for (int j = 0; j < NV4; ++j) {
                const int i = lane + 64 * j;
                if (i < nv) ctc_store4(g, 4 * i, V, make_float4(v[j].x * f, v[j].y * f, v[j].z * f, v[j].w * f));
            }
        }
    } else {
        m = NEG_INF;
        for (int i = lane; i < V; i += 64) m = fmaxf(m, p[i]);
        m = wave_max(m);
        float s = 0.f;
        for (int i = lane; i < V; i += 64) s += __expf(p[i] - m);
        s = wave_sum(s);
        l2s = __builtin_amdgcn_logf(s);
        if (WRITE) {
            const float f = scale / s;
            for (int i = lane; i < V; i += 64) g[i] = __expf(p[i] - m) * f;
        }
    }
#pragma unroll
    for (int q = 0; q < CTC_MAXQ; ++q) {
        const int st = lane + 64 * q;
        if (st < S) lp_out[row * Sp + st] = (lv[q] - m) * 1.4426950408889634f - l2s;
    }
}

// ------------------------------------------------------------------ k2 ------
// The recursion is one dependent chain per frame on a lone wave, so its cost is the chain's length.  Kept short by:
//  * base-2 logs throughout (lp, alpha, beta, ll are log2 values in the workspace): exp / log are the bare v_exp_f32 /
//    v_log_f32, no scaling multiplies and none of logf's denormal handling (the argument of the log is in [1, 3]);
//  * a finite "log 0" (CTC_NEG) instead of -inf: max - max is 0 and never NaN, so there is no guard in the chain;
//    CTC_NEG + anything the recursion adds stays CTC_NEG in fp32 (ulp(1e30) = 7.6e22);
//  * neighbours through DPP wave shifts (one VALU move) instead of ds_bpermute round trips;
//  * the direction is a template parameter of the recursion, not a per-step branch.
#define CTC_NEG (-1.0e30f)
#define CTC_LOG2E 1.4426950408889634f
#define CTC_LN2 0.6931471805599453f

__device__ __forceinline__ float ctc_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float ctc_log2(float x) { return __builtin_amdgcn_logf(x); }
// lane i <- lane i-1 (lane 0 <- CTC_NEG) / lane i <- lane i+1 (lane 63 <- CTC_NEG)
__device__ __forceinline__ float wave_shr1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, CTC_NEG), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shl1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, CTC_NEG), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
// log2(2^a + 2^b + 2^c) + add
__device__ __forceinline__ float lse3_add(float a, float b, float c, float add) {
    const float m = fmaxf(a, fmaxf(b, c));
    return ctc_log2(ctc_exp2(a - m) + ctc_exp2(b - m) + ctc_exp2(c - m)) + (m + add);
}

// One direction of the recursion for utterance rows [base, base + Tb): NS states per lane; CH frames of lp are fetched
// at a time, one chunk ahead.  Returns this lane's final values in a[].
template <bool FWD, int NS, int CH, bool FULL>
__device__ __forceinline__ void ctc_chunk(int c0, int Tb, const long (&ostr)[NS], float (&a)[NS], const float (&cap)[NS],
                                          const float (&cur)[CH][NS], float* (&op)[NS]) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (FULL || c0 + i < Tb) {       // wave-uniform; whole chunks carry no test
            // neighbour lane's nearest / second nearest state
            const float p1 = FWD ? wave_shr1(a[NS - 1]) : wave_shl1(a[0]);
            const float p2 = FWD ? (NS >= 2 ? wave_shr1(a[NS >= 2 ? NS - 2 : 0]) : wave_shr1(p1))
                                 : (NS >= 2 ? wave_shl1(a[NS >= 2 ? 1 : 0]) : wave_shl1(p1));
            float na[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                float n1, n2;
                if (FWD) {
                    n1 = (j >= 1) ? a[j >= 1 ? j - 1 : 0] : p1;
                    n2 = (j >= 2) ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2);
                } else {
                    n1 = (j + 1 < NS) ? a[j + 1 < NS ? j + 1 : 0] : p1;
                    n2 = (j + 2 < NS) ? a[j + 2 < NS ? j + 2 : 0] : (j + 1 < NS ? p1 : p2);
                }
                na[j] = lse3_add(a[j], n1, fminf(n2, cap[j]), cur[i][j]);
            }
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                a[j] = na[j];
                op[j] += ostr[j];
                *op[j] = a[j];
            }
        }
    }
}

// One direction of the recursion for utterance rows [base, base + Tb): NS states per lane; CH frames of lp are fetched
// at a time, one chunk ahead.  Returns this lane's final values in a[].  dump: one float any lane may scribble on.
// k0, k1: the steps this call runs, [k0, k1) of the utterance's Tb (step k works on frame FWD ? k : Tb-1-k).  k0 = 0 starts
// the recursion (first column); k0 > 0 resumes it from the values step k0 - 1 left in out_rows (an earlier launch).
template <bool FWD, int NS, int CH>
__device__ __forceinline__ void ctc_recurse(int lane, int Tb, int S, int Sp, const int* __restrict__ tg, const float* __restrict__ lp_rows,
                                            float* __restrict__ out_rows, float* __restrict__ dump, float (&a)[NS], int k0, int k1) {
    const int s0 = lane * NS;
    float cap[NS];   // upper bound on the s-2 (alpha) / s+2 (beta) term: that transition exists only between different labels
    bool valid[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int s = s0 + j;
        valid[j] = s < S;
        bool skip = false;
        if (s < S && (s & 1)) {
            if (FWD) { if (s >= 2) skip = tg[s >> 1] != tg[(s - 2) >> 1]; }
            else { if (s + 2 < S) skip = tg[s >> 1] != tg[(s + 2) >> 1]; }
        }
        cap[j] = skip ? 3.0e38f : CTC_NEG;
    }
    // step k of the recursion works on frame  FWD ? k : Tb-1-k
    const long tstride = FWD ? (long)Sp : -(long)Sp;
    const float* lp0 = lp_rows + (long)(FWD ? 0 : Tb - 1) * Sp + s0;      // frame of step 0, this lane's first state
    // states past S store to the dump word with stride 0: the stores of a step need no predicate
    const int kfirst = k0 > 0 ? k0 - 1 : 0;              // the step whose values a[] holds before the loop
    float* op[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) op[j] = valid[j] ? out_rows + (long)(FWD ? 0 : Tb - 1) * Sp + kfirst * tstride + s0 + j : dump;
    long ostr[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) ostr[j] = valid[j] ? tstride : 0;
    if (k0 == 0) {
        // ---- first column
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int s = s0 + j;
            const bool start = FWD ? (s <= 1) : (s >= S - 2);
            a[j] = CTC_NEG;
            if (valid[j] && start) a[j] = lp0[j];
            *op[j] = a[j];
        }
    } else {
        // ---- resume: the previous launch's last column
#pragma unroll
        for (int j = 0; j < NS; ++j) a[j] = valid[j] ? *op[j] : CTC_NEG;
    }
    const int kb = kfirst + 1;                             // first step of the loop
    // ---- recursion, steps 1 .. Tb-1 in chunks of CH.  States past S carry lp = 0: they stay CTC_NEG (beta's flow is
    // from high s to low s, so they must), and their values go to the dump word.
    float cur[CH][NS], nxt[CH][NS];
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            cur[i][j] = 0.f;
            if (kb + i < k1 && valid[j]) cur[i][j] = lp0[(kb + i) * tstride + j];
        }
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) asm volatile("" : "+v"(cur[i][j]));
    for (int c0 = kb; c0 < k1; c0 += CH) {
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                nxt[i][j] = 0.f;
                if (c0 + CH + i < k1 && valid[j]) nxt[i][j] = lp0[(c0 + CH + i) * tstride + j];
            }
        if (c0 + CH <= k1) ctc_chunk<FWD, NS, CH, true>(c0, k1, ostr, a, cap, cur, op);
        else ctc_chunk<FWD, NS, CH, false>(c0, k1, ostr, a, cap, cur, op);
        // the next chunk becomes current HERE: pinning the values makes the compiler wait for the prefetch once per
        // chunk.  Left to itself it waits lazily at each step's first use of a prefetched register, and with the steps'
        // stores in between that wait is vmcnt(0): every step then sits out its own store's acknowledgement
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                cur[i][j] = nxt[i][j];
                asm volatile("" : "+v"(cur[i][j]));
            }
    }
}

// chain[b][s] for odd s = (next state with the same label, + 1; 0 = none) | (first of its label ? 1 << 16 : 0): the states
// that share a class (a label occurring more than once in the target), linked once per utterance by one wave.  k3 follows
// these chains per frame instead of comparing labels (that comparison was O(S^2) per frame).
__device__ __forceinline__ void ctc_link_chains(int lane, int S, const int* __restrict__ tg, int* __restrict__ chain_b) {
    for (int s = 1 + 2 * lane; s < S; s += 128) {
        const int c = tg[s >> 1];
        int head = 1, nx = 0;
        for (int q = 1; q < s; q += 2) if (tg[q >> 1] == c) { head = 0; break; }
        for (int q = s + 2; q < S; q += 2) if (tg[q >> 1] == c) { nx = q + 1; break; }
        chain_b[s] = nx | (head << 16);
    }
}

// One block of three waves per utterance: wave 0 runs alpha, wave 1 beta, and wave 2 meanwhile links the label chains.
template <int NS, int CH>
__global__ __launch_bounds__(192) void ctc_alphabeta_kernel(int T, const int* __restrict__ hlens, const int* __restrict__ targets,
                                                            int Lmax, const int* __restrict__ tlens, int Sp,
                                                            const float* __restrict__ lp, float* __restrict__ alpha,
                                                            float* __restrict__ beta, float* __restrict__ ll_out,
                                                            float* __restrict__ nll_out, int* __restrict__ chain,
                                                            float* __restrict__ dump) {
    __shared__ float fin[2];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Tb = min(hlens[b], T);
    const int S = 2 * min(tlens[b], Lmax) + 1;
    const int* tg = targets + (long)b * Lmax;
    const long base = (long)b * T * Sp;
    if (threadIdx.x < 2) fin[threadIdx.x] = CTC_NEG;
    __syncthreads();
    if (wv == 2) {
        ctc_link_chains(lane, S, tg, chain + (long)b * Sp);
    } else if (Tb > 0 && wv < 2) {      // (wv < 2 always holds in a block of three waves)
        float a[NS];
        if (wv == 0) {
            ctc_recurse<true, NS, CH>(lane, Tb, S, Sp, tg, lp + base, alpha + base, dump, a, 0, Tb);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (lane * NS + j == S - 1) fin[0] = a[j];
                if (lane * NS + j == S - 2) fin[1] = a[j];
            }
        } else {
            ctc_recurse<false, NS, CH>(lane, Tb, S, Sp, tg, lp + base, beta + base, dump, a, 0, Tb);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // log2-likelihood; anything that still carries the CTC_NEG scale is an infeasible alignment:
        // zero_infinity makes it contribute 0 loss and 0 gradient
        float ll = NEG_INF;
        if (Tb > 0) {
            const float m = fmaxf(fin[0], fin[1]);
            const float v = m + ctc_log2(ctc_exp2(fin[0] - m) + ctc_exp2(fin[1] - m));
            if (v > 0.5f * CTC_NEG) ll = v;
        }
        ll_out[b] = ll;                                        // base 2, for k3
        nll_out[b] = (ll == NEG_INF) ? 0.f : -ll * CTC_LN2;
    }
}

// ---- the pipelined form (oe_ctc_loss_fused with T >= CTC_PIPE_MIN_T): the recursion in time chunks, one direction per launch.
// One wave per utterance runs its direction over the frames [t0, t1) of the chunk: alpha resumes from the column the
// previous chunk's launch left at frame t0 - 1, beta from frame t1; the launch that reaches the utterance's last frame
// (alpha) also publishes the log-likelihood.  The host queues alpha chunks 0, 1, .. on one stream and beta chunks NC-1, NC-2,
// .. on another, each behind the `rows` launch that produced its frames (ordinary stream events), so both chains run under
// the remaining `rows` traffic instead of after it.
template <bool FWD, int NS, int CH>
__global__ __launch_bounds__(64) void ctc_dir_kernel(int T, int t0, int t1, const int* __restrict__ hlens, const int* __restrict__ targets,
                                                     int Lmax, const int* __restrict__ tlens, int Sp, const float* __restrict__ lp,
                                                     float* __restrict__ state, float* __restrict__ ll_out, float* __restrict__ nll_out,
                                                     float* __restrict__ dump) {
    __shared__ float fin[2];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = min(hlens[b], T);
    const int S = 2 * min(tlens[b], Lmax) + 1;
    const int* tg = targets + (long)b * Lmax;
    const long base = (long)b * T * Sp;
    if (FWD && Tb == 0 && t0 == 0 && lane == 0) { ll_out[b] = NEG_INF; nll_out[b] = 0.f; }
    const int f1 = min(t1, Tb);                       // frames [t0, f1) of this utterance lie in the chunk
    if (t0 >= f1) return;
    const int k0 = FWD ? t0 : Tb - f1, k1 = FWD ? f1 : Tb - t0;
    float a[NS];
    ctc_recurse<FWD, NS, CH>(lane, Tb, S, Sp, tg, lp + base, state + base, dump, a, k0, k1);
    if (FWD && f1 == Tb) {                            // the last frame: log2-likelihood (see ctc_alphabeta_kernel)
        if (lane < 2) fin[lane] = CTC_NEG;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (lane * NS + j == S - 1) fin[0] = a[j];
            if (lane * NS + j == S - 2) fin[1] = a[j];
        }
        __syncthreads();
        if (lane == 0) {
            const float m = fmaxf(fin[0], fin[1]);
            const float v = m + ctc_log2(ctc_exp2(fin[0] - m) + ctc_exp2(fin[1] - m));
            const float ll = (v > 0.5f * CTC_NEG) ? v : NEG_INF;
            ll_out[b] = ll;
            nll_out[b] = (ll == NEG_INF) ? 0.f : -ll * CTC_LN2;
        }
    }
}
// chain[b][s] for odd s (see ctc_alphabeta_kernel): one wave per utterance
__global__ __launch_bounds__(64) void ctc_chain_kernel(const int* __restrict__ targets, int Lmax, const int* __restrict__ tlens, int Sp,
                                                       int* __restrict__ chain) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int S = 2 * min(tlens[b], Lmax) + 1;
    ctc_link_chains(lane, S, targets + (long)b * Lmax, chain + (long)b * Sp);
}

// ------------------------------------------------------------------ k3 ------
// One wave per frame (four per block).  k1 has written softmax * scale everywhere; the classes of the target get their
// occupation term here, and frames of an infeasible utterance (ll = -inf) are zeroed.  Block 0 also sums the loss.
// Sums run in a fixed order (blank: per-lane partials + shuffle tree; a label: along its chain): deterministic.
// ST: the type of alpha, beta and ll - float, or double on the long-launch path, where the exponent is formed in float64
template <typename ST>
__device__ __forceinline__ void ctc_labels_block(float* sh, long blk, long rows, int B, int T, int V, long ldv, const int* __restrict__ hlens,
                                                 const int* __restrict__ targets, int Lmax, const int* __restrict__ tlens,
                                                 int Sp, const float* __restrict__ lp, const ST* __restrict__ alpha,
                                                 const ST* __restrict__ beta, const ST* __restrict__ ll_in,
                                                 const int* __restrict__ chain, const float* __restrict__ nll,
                                                 float scale, const float* __restrict__ utt_weight,
                                                 float* __restrict__ dlogits, float* __restrict__ loss_sum, int t0, int Tc) {
    // frames t0 .. t0 + Tc - 1 of every utterance (`rows` = B * Tc; the whole batch: t0 = 0, Tc = T); sh: per wave gam[Sp]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (loss_sum && blk == 0 && wv == 0) {
        float s = 0.f;
        for (int i = lane; i < B; i += 64) s += utt_weight ? nll[i] * utt_weight[i] : nll[i];
        s = wave_sum(s);
        if (lane == 0) loss_sum[0] = s;
    }
    const long rloc = blk * 4 + wv;
    const bool inrange = rloc < rows;
    const int b = inrange ? (int)(rloc / Tc) : 0, t = inrange ? t0 + (int)(rloc % Tc) : 0;
    const long row = (long)b * T + t;
    const bool frame = inrange && t < hlens[b];
    const ST ll = ll_in[b];
    float* g = dlogits + row * ldv;
    if (frame && ll == NEG_INF) {
        for (int i = lane; i < V; i += 64) g[i] = 0.f;
    }
    const bool live = frame && ll != NEG_INF;
    if (utt_weight) scale *= utt_weight[b];
    const int S = live ? 2 * min(tlens[b], Lmax) + 1 : 0;
    float* gam = sh + (size_t)wv * Sp;
    const float* lpr = lp + row * Sp;
    float blank = 0.f, own[CTC_MAXQ];
#pragma unroll
    for (int q = 0; q < CTC_MAXQ; ++q) {
        const int s = lane + 64 * q;
        own[q] = 0.f;
        if (s < S) {
            const long o = row * Sp + s;
            own[q] = lpr[s];
            const float gm = __builtin_amdgcn_exp2f((float)(alpha[o] + beta[o] - (ST)own[q] - ll));
            gam[s] = gm;
            if (!(s & 1)) blank += gm;
        }
    }
    blank = wave_sum(blank);
    __syncthreads();
    if (live && lane == 0) g[0] = (__builtin_amdgcn_exp2f(own[0]) - blank) * scale;
    const int* ch = chain + (long)b * Sp;
#pragma unroll
    for (int q = 0; q < CTC_MAXQ; ++q) {
        const int s = lane + 64 * q;
        if (s < S && (s & 1)) {
            int info = ch[s];
            if (info >> 16) {
                float occ = gam[s];
                for (int nx = (info & 0xffff) - 1; nx >= 0; nx = (ch[nx] & 0xffff) - 1) occ += gam[nx];
                g[targets[(long)b * Lmax + (s >> 1)]] = (__builtin_amdgcn_exp2f(own[q]) - occ) * scale;
            }
        }
    }
}
__global__ __launch_bounds__(256) void ctc_labels_kernel(long rows, int B, int T, int V, long ldv, const int* __restrict__ hlens,
                                                          const int* __restrict__ targets, int Lmax, const int* __restrict__ tlens,
                                                          int Sp, const float* __restrict__ lp, const float* __restrict__ alpha,
                                                          const float* __restrict__ beta, const float* __restrict__ ll_in,
                                                          const int* __restrict__ chain, const float* __restrict__ nll,
                                                          float scale, const float* __restrict__ utt_weight,
                                                          float* __restrict__ dlogits, float* __restrict__ loss_sum, int t0, int Tc) {
    extern __shared__ __attribute__((aligned(16))) float sh[];   // per wave: gam[Sp]
    ctc_labels_block<float>(sh, blockIdx.x, rows, B, T, V, ldv, hlens, targets, Lmax, tlens, Sp, lp, alpha, beta, ll_in, chain, nll, scale,
                            utt_weight, dlogits, loss_sum, t0, Tc);
}
// ---- the float64-state path (launches with T > ctc_f32_max_t, see there): k1 as above, then k2 / k3 with alpha, beta and ll in
// float64.  The recursion is ctc_f64.h's (the n-best scorer's); the exponent of an occupancy is formed in float64, so its error
// no longer grows with |ll|.  One block per utterance: wave 0 alpha, wave 1 beta, wave 2 the label chains.
template <int NS, int CH>
__global__ __launch_bounds__(192) void ctc_alphabeta_f64_kernel(int T, const int* __restrict__ hlens, const int* __restrict__ targets,
                                                                int Lmax, const int* __restrict__ tlens, int Sp,
                                                                const float* __restrict__ lp, double* __restrict__ alpha,
                                                                double* __restrict__ beta, double* __restrict__ ll_out,
                                                                float* __restrict__ nll_out, int* __restrict__ chain,
                                                                double* __restrict__ dump) {
    __shared__ double fin[2];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int Tb = min(hlens[b], T);
    const int S = 2 * min(tlens[b], Lmax) + 1;
    const int* tg = targets + (long)b * Lmax;
    const long base = (long)b * T * Sp;
    if (threadIdx.x < 2) fin[threadIdx.x] = NB_NEG_D;
    __syncthreads();
    if (wv == 2) {
        ctc_link_chains(lane, S, tg, chain + (long)b * Sp);
    } else if (Tb > 0) {
        double a[NS];
        if (wv == 0) {
            nb_recurse<true, NS, CH>(lane, Tb, S, Sp, tg, lp + base, alpha + base, dump, a);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (lane * NS + j == S - 1) fin[0] = a[j];
                if (lane * NS + j == S - 2) fin[1] = a[j];
            }
        } else {
            nb_recurse<false, NS, CH>(lane, Tb, S, Sp, tg, lp + base, beta + base, dump + 1, a);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // as ctc_alphabeta_kernel: anything that still carries the "log 0" scale is an infeasible alignment
        double ll = -INFINITY;
        if (Tb > 0) {
            const double m = fmax(fin[0], fin[1]);
            const double v = m + (double)nb_log2(nb_exp2((float)(fin[0] - m)) + nb_exp2((float)(fin[1] - m)));
            if (v > 0.5 * NB_NEG_D) ll = v;
        }
        ll_out[b] = ll;                                        // base 2, for k3
        nll_out[b] = (ll == -INFINITY) ? 0.f : (float)(-ll * 0.69314718055994530942);
    }
}
__global__ __launch_bounds__(256) void ctc_labels_f64_kernel(long rows, int B, int T, int V, long ldv, const int* __restrict__ hlens,
                                                              const int* __restrict__ targets, int Lmax, const int* __restrict__ tlens,
                                                              int Sp, const float* __restrict__ lp, const double* __restrict__ alpha,
                                                              const double* __restrict__ beta, const double* __restrict__ ll_in,
                                                              const int* __restrict__ chain, const float* __restrict__ nll,
                                                              float scale, const float* __restrict__ utt_weight,
                                                              float* __restrict__ dlogits, float* __restrict__ loss_sum) {
    extern __shared__ __attribute__((aligned(16))) float sh[];   // per wave: gam[Sp]
    ctc_labels_block<double>(sh, blockIdx.x, rows, B, T, V, ldv, hlens, targets, Lmax, tlens, Sp, lp, alpha, beta, ll_in, chain, nll,
                             scale, utt_weight, dlogits, loss_sum, 0, T);
}

__global__ void ctc_sum_kernel(const float* __restrict__ nll, const float* __restrict__ utt_weight, int B, float* __restrict__ out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 64) s += utt_weight ? nll[i] * utt_weight[i] : nll[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[0] = s;
}

// Streams and events of the pipelined form, one set per device, made on first use (a first use is never inside a graph
// capture: the engine runs an eager step before it captures).  Re-recording an event does not disturb waits already queued.
#define CTC_MAX_CHUNKS 8
#define OE_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { oe_set_error("oe_ctc_loss_fused: %s", hipGetErrorString(e_)); return (int)e_; } } while (0)
struct CtcPipe {
    hipStream_t sa = nullptr, sb = nullptr;
    hipEvent_t rows_done[CTC_MAX_CHUNKS], beta_done[CTC_MAX_CHUNKS], alpha_done;
    bool ok = false;
};
static CtcPipe* ctc_pipe() {
    static CtcPipe pipes[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    CtcPipe& p = pipes[dev];
    if (!p.ok) {
        if (hipStreamCreateWithFlags(&p.sa, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&p.sb, hipStreamNonBlocking) != hipSuccess) return nullptr;
        for (int i = 0; i < CTC_MAX_CHUNKS; ++i) {
            if (hipEventCreateWithFlags(&p.rows_done[i], hipEventDisableTiming) != hipSuccess) return nullptr;
            if (hipEventCreateWithFlags(&p.beta_done[i], hipEventDisableTiming) != hipSuccess) return nullptr;
        }
        if (hipEventCreateWithFlags(&p.alpha_done, hipEventDisableTiming) != hipSuccess) return nullptr;
        p.ok = true;
    }
    return &p;
}

// OE_CTC_PIPE: 0 = rows, alpha/beta, labels one after the other (default); 1 / 2 = chunk pipeline on two streams where the batch
// is large enough / always; OE_CTC_CHUNKS: its time chunks.  The pipeline is bit-for-bit equal (tests run it) and measured SLOWER
// than the default on MI355X (tools/ctc_graph_bench.py, profiles/r03_experiments.md): every cross-stream edge costs more than the
// chain time it hides - from a HIP graph 216 us sequential against 335 / 352 / 384 / 436 us with 2 / 3 / 4 / 6 chunks at the
// north-star shape (eager launches: 209 against 310 with 4) - so it is not the default.
// An overlapped form (row statistics first, then mixed launches of recursion / fix-up blocks beside dense-gradient blocks; modes
// 3 / 4) was also measured slower, 294 us against 208, and removed: profiles/r03_experiments.md.
static int ctc_pipe_mode = getenv("OE_CTC_PIPE") ? atoi(getenv("OE_CTC_PIPE")) : 0;
static int ctc_pipe_chunks = getenv("OE_CTC_CHUNKS") ? atoi(getenv("OE_CTC_CHUNKS")) : 4;
extern "C" int oe_ctc_config(int pipe_mode, int chunks) {
    if (pipe_mode >= 0) ctc_pipe_mode = pipe_mode;
    if (chunks >= 2) ctc_pipe_chunks = chunks;
    return 0;
}

// Launches with T above this run alpha / beta / ll in float64 (ctc_alphabeta_f64_kernel), the others in float32.  In float32
// every step of the recursion rounds a state of magnitude ~|ll|, and an occupancy 2^(alpha + beta - lp - ll) inherits that error
// in its exponent: the gradient's error grows with the utterance's negative log-likelihood, which for untrained (flat)
// posteriors grows with T.  The constant is the largest T of the ladder below at which, and below which, the float32 path
// meets the gradient tolerance 2e-5 + 2e-3 * |ref| against torch's CTC loss in float64 (tests/test_ctc_long_gpu.py::
// test_ladder: B = 1, V = 3246, randn * 2 logits, L = min(255, T / 6), seeds 0 - 2; worst err / tol over the seeds, MI355X):
//   T          248     400     600     800    1000    1500    2000
//   float32   0.70    1.48    3.25    3.98    8.42    9.16    49.7
//   float64  0.002   0.005   0.004   0.004   0.004   0.004   0.007
// (the loss itself is within 0.02 of its tolerance rtol 1e-4 / atol 1e-3 on both paths.)  Other shapes in float32: 617 at
// (T, V, L) = (1500, 64, 200) with randn * 6 logits (|nll| 15000 nats), 1430 at (2000, 32, 255) with randn * 8; float64 0.04 and 0.07.
// Posteriors peaked on an alignment (|nll| of a few nats) pass in float32 at any of these lengths: the error follows |nll|, not T.
// OE_CTC_F32_MAX_T overrides it (for measuring that table; a tuning knob like OE_CTC_PIPE).
#define CTC_F32_MAX_T 248
static int ctc_f32_max_t = getenv("OE_CTC_F32_MAX_T") ? atoi(getenv("OE_CTC_F32_MAX_T")) : CTC_F32_MAX_T;

extern "C" size_t oe_ctc_workspace_floats(int B, int T, int Lmax) {
    size_t Sp = 2 * (size_t)Lmax + 1;
    size_t n = (size_t)B + 3 * (size_t)B * T * Sp + (size_t)B * Sp + 16;          // ll, lp, alpha, beta, chain, 16 spare floats
    if (T > ctc_f32_max_t) n += 2 * (size_t)B * T * Sp + 2 * (size_t)B + 2;      // alpha, beta, ll in float64, 8-byte aligned
    return n;
}

// k1 over frames t0 .. t0 + tc - 1 of every utterance, for the loss (both state widths) and the aligner: the row variant the
// pointers and V allow, with the dense gradient when dlogits is given.
static void ctc_launch_rows(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* targets, int Lmax,
                            const int* tlens, int Sp, float scale, const float* utt_weight, float* lp, float* dlogits, int t0, int tc,
                            hipStream_t st) {
    const long rows = (long)B * tc;
    // register-resident rows need 16-byte aligned rows that are padded to whole float4s
    const bool vec = (((uintptr_t)logits & 15) == 0) && (!dlogits || ((uintptr_t)dlogits & 15) == 0) && (ldv % 4 == 0) &&
                     (ldv >= (((long)V + 3) & ~3L)) && V <= 256 * 32;
    const int nv4 = !vec ? 0 : V <= 256 * 4 ? 4 : V <= 256 * 8 ? 8 : V <= 256 * 16 ? 16 : 32;
#define ROWS(NV4, WR)                                                                                                            \
    hipLaunchKernelGGL((ctc_rows_kernel<NV4, WR>), dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, logits, ldv, rows, T, V, hlens, targets, \
                       Lmax, tlens, Sp, scale, utt_weight, lp, dlogits, t0, tc)
#define ROWS_W(NV4) do { if (dlogits) ROWS(NV4, true); else ROWS(NV4, false); } while (0)
    switch (nv4) {
        case 4: ROWS_W(4); break;
        case 8: ROWS_W(8); break;
        case 16: ROWS_W(16); break;
        case 32: ROWS_W(32); break;
        default: ROWS_W(0); break;
    }
#undef ROWS_W
#undef ROWS
}

extern "C" int oe_ctc_loss_fused(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* targets,
                                 int Lmax, const int* tlens, float grad_scale, const float* utt_weight, float* nll,
                                 float* loss_sum, float* dlogits, float* workspace, void* stream) {
    OE_REQUIRE(logits && hlens && tlens && nll && workspace, "oe_ctc_loss_fused: null pointer");
    OE_REQUIRE(targets || Lmax == 0, "oe_ctc_loss_fused: null targets");
    OE_REQUIRE(B > 0 && T > 0 && V > 1 && Lmax >= 0 && ldv >= V, "oe_ctc_loss_fused: bad shape B=%d T=%d V=%d Lmax=%d ldv=%ld",
               B, T, V, Lmax, ldv);
    const int Sp = 2 * Lmax + 1;
    OE_REQUIRE(Sp <= 64 * CTC_MAXQ, "oe_ctc_loss_fused: target length %d exceeds the 255-label limit of the wave recursion", Lmax);
    hipStream_t st = (hipStream_t)stream;
    float* ll = workspace;
    float* lp = ll + B;
    float* alpha = lp + (size_t)B * T * Sp;
    float* beta = alpha + (size_t)B * T * Sp;
    int* chain = reinterpret_cast<int*>(beta + (size_t)B * T * Sp);
    float* dump = reinterpret_cast<float*>(chain + (size_t)B * Sp);      // the 16 spare floats at the end
    const long rows = (long)B * T;
    auto launch_rows = [&](int t0, int tc) {
        ctc_launch_rows(logits, ldv, B, T, V, hlens, targets, Lmax, tlens, Sp, grad_scale, utt_weight, lp, dlogits, t0, tc, st);
    };
    // ---- float64-state path (see ctc_f32_max_t): rows, alpha/beta, labels one after the other whatever the launch form asked for.
    // Workspace: ll (unused), lp, then chain, and behind it ll / alpha / beta / two dump words as doubles.
    if (T > ctc_f32_max_t) {
        int* chain64 = reinterpret_cast<int*>(alpha);
        double* ll64 = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(chain64 + (size_t)B * Sp) + 7) & ~(uintptr_t)7);
        double* alpha64 = ll64 + B;
        double* beta64 = alpha64 + (size_t)B * T * Sp;
        double* dump64 = beta64 + (size_t)B * T * Sp;
        launch_rows(0, T);
        OE_LAUNCH_CHECK("ctc_rows");
#define AB64(NS, CH) hipLaunchKernelGGL((ctc_alphabeta_f64_kernel<NS, CH>), dim3(B), dim3(192), 0, st, T, hlens, targets, Lmax, tlens, \
                                        Sp, lp, alpha64, beta64, ll64, nll, chain64, dump64)
        if (Sp <= 64) AB64(1, 32); else if (Sp <= 128) AB64(2, 16); else if (Sp <= 256) AB64(4, 8); else AB64(8, 4);
#undef AB64
        OE_LAUNCH_CHECK("ctc_alphabeta_f64");
        if (dlogits) {
            hipLaunchKernelGGL(ctc_labels_f64_kernel, dim3(oe_cdiv(rows, 4)), dim3(256), (size_t)4 * Sp * sizeof(float), st, rows, B, T, V, ldv, hlens,
                               targets, Lmax, tlens, Sp, lp, alpha64, beta64, ll64, chain64, nll, grad_scale, utt_weight, dlogits, loss_sum);
            OE_LAUNCH_CHECK("ctc_labels_f64");
        } else if (loss_sum) {
            hipLaunchKernelGGL(ctc_sum_kernel, dim3(1), dim3(64), 0, st, nll, utt_weight, B, loss_sum);
            OE_LAUNCH_CHECK("ctc_sum");
        }
        return 0;
    }
    auto launch_labels = [&](int t0, int tc, float* lsum) {
        hipLaunchKernelGGL(ctc_labels_kernel, dim3(oe_cdiv((long)B * tc, 4)), dim3(256), (size_t)4 * Sp * sizeof(float), st, (long)B * tc, B, T, V,
                           ldv, hlens, targets, Lmax, tlens, Sp, lp, alpha, beta, ll, chain, nll, grad_scale, utt_weight, dlogits, lsum, t0, tc);
    };
    // ---- pipelined form (opt-in, see ctc_pipe_mode): the recursion in time chunks under the remaining `rows` traffic
    // (ctc_dir_kernel) - rows 115 us, the two chains 60 us each, label fix-up 30 us at the 16 s north-star batch.
    const int pipe_mode = ctc_pipe_mode, pipe_chunks = ctc_pipe_chunks;
    CtcPipe* pp = nullptr;
    const int NC = min(max(pipe_chunks, 2), CTC_MAX_CHUNKS);
    if ((pipe_mode == 1 || pipe_mode == 2) && dlogits && (pipe_mode == 2 ? T >= 2 * NC : (T >= 32 * NC && (double)rows * V >= 1.5e7))) pp = ctc_pipe();
    if (pp) {
        const int Tq = oe_cdiv(T, NC);
        auto c0 = [&](int c) { return c * Tq; };
        auto cn = [&](int c) { return min(T, (c + 1) * Tq) - c * Tq; };
        hipLaunchKernelGGL(ctc_chain_kernel, dim3(B), dim3(64), 0, st, targets, Lmax, tlens, Sp, chain);
        // rows in the order first, last, second, second-to-last, ...: alpha needs the frames from the front, beta from the back
        int lo = 0, hi = NC - 1;
        for (int i = 0; i < NC; ++i) {
            const int c = (i & 1) ? hi-- : lo++;
            if (cn(c) > 0) launch_rows(c0(c), cn(c));
            OE_HIP(hipEventRecord(pp->rows_done[c], st));
        }
        OE_LAUNCH_CHECK("ctc_rows");
#define DIR(FWD, NS, CH, STR, C)                                                                                                   \
        hipLaunchKernelGGL((ctc_dir_kernel<FWD, NS, CH>), dim3(B), dim3(64), 0, STR, T, c0(C), c0(C) + cn(C), hlens, targets, Lmax, tlens, \
                           Sp, lp, (FWD) ? alpha : beta, ll, nll, dump + ((FWD) ? 0 : 8))
#define DIRS(FWD, STR, C) do { if (Sp <= 64) DIR(FWD, 1, 32, STR, C); else if (Sp <= 128) DIR(FWD, 2, 16, STR, C);                 \
                               else if (Sp <= 256) DIR(FWD, 4, 8, STR, C); else DIR(FWD, 8, 4, STR, C); } while (0)
        for (int c = 0; c < NC; ++c) {
            OE_HIP(hipStreamWaitEvent(pp->sa, pp->rows_done[c], 0));
            if (cn(c) > 0) DIRS(true, pp->sa, c);
        }
        OE_HIP(hipEventRecord(pp->alpha_done, pp->sa));
        for (int c = NC - 1; c >= 0; --c) {
            OE_HIP(hipStreamWaitEvent(pp->sb, pp->rows_done[c], 0));
            if (cn(c) > 0) DIRS(false, pp->sb, c);
            OE_HIP(hipEventRecord(pp->beta_done[c], pp->sb));
        }
#undef DIRS
#undef DIR
        OE_LAUNCH_CHECK("ctc_dir");
        // label fix-up per chunk once both directions have passed it (the log-likelihood comes with the end of alpha)
        OE_HIP(hipStreamWaitEvent(st, pp->alpha_done, 0));
        for (int c = NC - 1; c >= 0; --c) {
            OE_HIP(hipStreamWaitEvent(st, pp->beta_done[c], 0));
            if (cn(c) > 0) launch_labels(c0(c), cn(c), c == 0 ? loss_sum : nullptr);      // chunk 0 is last: every nll is final
        }
        OE_LAUNCH_CHECK("ctc_labels");
        return 0;
    }
    launch_rows(0, T);
    OE_LAUNCH_CHECK("ctc_rows");
#define AB(NS, CH) hipLaunchKernelGGL((ctc_alphabeta_kernel<NS, CH>), dim3(B), dim3(192), 0, st, T, hlens, targets, Lmax, tlens, \
                                      Sp, lp, alpha, beta, ll, nll, chain, dump)
    if (Sp <= 64) AB(1, 32); else if (Sp <= 128) AB(2, 16); else if (Sp <= 256) AB(4, 8); else AB(8, 4);
#undef AB
    OE_LAUNCH_CHECK("ctc_alphabeta");
    if (dlogits) {
        launch_labels(0, T, loss_sum);
        OE_LAUNCH_CHECK("ctc_labels");
    } else if (loss_sum) {
        hipLaunchKernelGGL(ctc_sum_kernel, dim3(1), dim3(64), 0, st, nll, utt_weight, B, loss_sum);
        OE_LAUNCH_CHECK("ctc_sum");
    }
    return 0;
}

// ------------------------------------------------------------- greedy -------
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, long ldv, long rows, int V,
                                                           int* __restrict__ best) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = x + row * ldv;
    float bv = NEG_INF;
    int bi = 0x7fffffff;
    for (int i = lane; i < V; i += 64) {
        float v = p[i];
        if (v > bv || bi == 0x7fffffff) { bv = v; bi = i; }   // strictly greater: lowest index kept inside a lane
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        float ov = __shfl_xor(bv, o, 64);
        int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) best[row] = bi;
}

__global__ __launch_bounds__(64) void ctc_collapse_kernel(const int* __restrict__ best, int T, const int* __restrict__ hlens,
                                                           int eos, int* __restrict__ out_tokens, int* __restrict__ out_lens) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int hl = hlens[b];
    const int* row = best + (long)b * T;
    int* out = out_tokens + (long)b * T;
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        int cur = 0, prev = -1;
        if (t < T) {
            cur = (t < hl) ? row[t] : eos;
            if (t > 0) prev = (t - 1 < hl) ? row[t - 1] : eos;
        }
        const bool keep = (t < T) && (cur != 0) && (cur != prev);
        const unsigned long long mask = __ballot(keep);
        const int pos = n + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep) out[pos] = cur;
        n += __popcll(mask);
    }
    for (int t = n + lane; t < T; t += 64) out[t] = -1;
    if (lane == 0) out_lens[b] = n;
}

extern "C" int oe_ctc_greedy(const float* logits, long ldv, int B, int T, int V, const int* hlens, int eos,
                             int* frame_best, int* out_tokens, int* out_lens, void* stream) {
    OE_REQUIRE(logits && hlens && frame_best && out_tokens && out_lens, "oe_ctc_greedy: null pointer");
    OE_REQUIRE(B > 0 && T > 0 && V > 0 && ldv >= V, "oe_ctc_greedy: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * T;
    hipLaunchKernelGGL(argmax_rows_kernel, dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, logits, ldv, rows, V, frame_best);
    OE_LAUNCH_CHECK("argmax_rows");
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(64), 0, st, frame_best, T, hlens, eos, out_tokens, out_lens);
    OE_LAUNCH_CHECK("ctc_collapse");
    return 0;
}

// ------------------------------------------------------- forced alignment ----
// The max-product twin of the alpha recursion: the best path through the trellis of ctc.py:27-45 (blank, y1, blank, .. blank;
// skip between different labels only) instead of the sum over all of them.  The reference has no aligner; the semantics
// (tie rule included) are in include/openeat_hip.h.
//   launch 1: ctc_rows_kernel<NV4, false>, exactly as the loss-only path: lp[b,t,s] = log2-prob at the 2L+1 states
//   launch 2: ctc_align_kernel, one wave per utterance:
//     recursion  v[t,s] = lp[t,s] + max(stay, step, skip), states NS per lane, neighbours by the DPP shifts, lp prefetched a
//                chunk ahead - ctc_recurse<true> with max for the log-sum-exp.  Each step also leaves one word per lane: the
//                moves of its NS states, 2 bits each (0 stay / 1 step / 2 skip).  A lane only ever reads back its own words,
//                so they are private storage and need no fence: in LDS (one byte per lane and frame for NS <= 4, two for
//                NS = 8) while T * 64 of them fit CTC_ALIGN_LDS = 60 KiB - the 64 KiB a launch may ask for without a
//                per-function opt-in, less the span table - i.e. T <= 960 (Sp <= 256) or T <= 480 (Sp <= 512); in the
//                workspace for longer batches (the route depends on T and Sp only, not on the data).
//     back-trace the whole wave walks from Tb-1 to 0 with the state in a scalar register: every lane loads its word of a
//                frame (addresses do not depend on the path: 16 frames in flight), v_readlane picks the current state's, so
//                a step of the chain is a readlane, a shift and a subtract.  Lane t & 63 keeps (state, move) of frame t;
//                after 64 frames the wave writes that tile of `frames` and marks the spans' first / last frames in LDS.
//     spans      one lane per label: start, end, and the sum of lp over the span (a fixed order: deterministic).
// Bound: a latency chain of Tb dependent steps on one wave, like alphabeta; the back-trace adds a shorter chain of Tb.
#define CTC_ALIGN_LDS (60 * 1024)
#define CTC_ALIGN_PF 16          // frames of back-pointers in flight during the back-trace

template <int NS, int CH, bool FULL, typename BPT>
__device__ __forceinline__ void ctc_align_chunk(int c0, int Tb, float (&a)[NS], const float (&cap)[NS], const float (&cur)[CH][NS], BPT* bpl) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (FULL || c0 + i < Tb) {       // wave-uniform; whole chunks carry no test
            const float p1 = wave_shr1(a[NS - 1]);
            const float p2 = NS >= 2 ? wave_shr1(a[NS >= 2 ? NS - 2 : 0]) : wave_shr1(p1);
            float na[NS];
            unsigned w = 0;
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const float n1 = (j >= 1) ? a[j >= 1 ? j - 1 : 0] : p1;
                const float n2 = fminf((j >= 2) ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2), cap[j]);
                // a predecessor replaces the best only if strictly greater, in the order stay, step, skip
                float best = a[j];
                unsigned mv = 0;
                if (n1 > best) { best = n1; mv = 1; }
                if (n2 > best) { best = n2; mv = 2; }
                na[j] = best + cur[i][j];
                w |= mv << (2 * j);
            }
#pragma unroll
            for (int j = 0; j < NS; ++j) a[j] = na[j];
            bpl[(size_t)(c0 + i) * 64] = (BPT)w;
        }
    }
}

// bpl: this lane's column of the back-pointer words, word of frame t at bpl[t * 64] (LDS or workspace)
template <int NS, int CH, typename BPT>
__device__ __forceinline__ void ctc_align_wave(BPT* bpl, int* __restrict__ span, int b, int T, int Tb, int L, int Lmax, int Sp,
                                               const int* __restrict__ tg, const float* __restrict__ lp_rows, int* __restrict__ frames,
                                               int* __restrict__ tok_start, int* __restrict__ tok_end, float* __restrict__ tok_logp,
                                               float* __restrict__ score) {
    const int lane = threadIdx.x;
    const int S = 2 * L + 1;
    const int s0 = lane * NS;
    int* fr = frames + (long)b * T;
    float sc = NEG_INF;
    bool feasible = false;
    for (int l = lane; l < 2 * Lmax; l += 64) span[l] = -1;            // [0, Lmax): first frames, [Lmax, 2 Lmax): last frames
    if (Tb > 0) {
        // ---- recursion (see ctc_recurse: finite "log 0", states past S carry lp = 0 and never feed a valid state)
        float cap[NS], a[NS];
        bool valid[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int s = s0 + j;
            valid[j] = s < S;
            const bool skip = s < S && (s & 1) && s >= 3 && tg[s >> 1] != tg[(s - 2) >> 1];
            cap[j] = skip ? 3.0e38f : CTC_NEG;
        }
        const float* lp0 = lp_rows + s0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            a[j] = CTC_NEG;
            if (valid[j] && s0 + j <= 1) a[j] = lp0[j];
        }
        float cur[CH][NS], nxt[CH][NS];
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                cur[i][j] = 0.f;
                if (1 + i < Tb && valid[j]) cur[i][j] = lp0[(long)(1 + i) * Sp + j];
            }
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) asm volatile("" : "+v"(cur[i][j]));
        for (int c0 = 1; c0 < Tb; c0 += CH) {
#pragma unroll
            for (int i = 0; i < CH; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    nxt[i][j] = 0.f;
                    if (c0 + CH + i < Tb && valid[j]) nxt[i][j] = lp0[(long)(c0 + CH + i) * Sp + j];
                }
            if (c0 + CH <= Tb) ctc_align_chunk<NS, CH, true>(c0, Tb, a, cap, cur, bpl);
            else ctc_align_chunk<NS, CH, false>(c0, Tb, a, cap, cur, bpl);
            // the next chunk becomes current here, one wait per chunk (see ctc_recurse)
#pragma unroll
            for (int i = 0; i < CH; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    cur[i][j] = nxt[i][j];
                    asm volatile("" : "+v"(cur[i][j]));
                }
        }
        // ---- end state: 2L unless 2L-1 is strictly greater
        float e0 = CTC_NEG, e1 = CTC_NEG;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (s0 + j == S - 1) e0 = a[j];
            if (s0 + j == S - 2) e1 = a[j];
        }
        e0 = wave_max(e0);
        e1 = wave_max(e1);
        const float best = (e1 > e0) ? e1 : e0;
        feasible = best > 0.5f * CTC_NEG;
        if (feasible) {
            sc = best * CTC_LN2;
            // ---- back-trace
            int s = __builtin_amdgcn_readfirstlane((e1 > e0) ? S - 2 : S - 1);
            int above = -1;                                  // state of the frame after the tile in hand
            for (int t0 = (Tb - 1) & ~63; t0 >= 0; t0 -= 64) {
                const int thi = min(Tb - 1, t0 + 63);
                int myS = -1, myMv = 0;
                for (int g = thi; g >= t0; g -= CTC_ALIGN_PF) {
                    unsigned w[CTC_ALIGN_PF];
#pragma unroll
                    for (int k = 0; k < CTC_ALIGN_PF; ++k) {
                        const int t = g - k;
                        w[k] = 0u;
                        if (t >= t0 && t >= 1) w[k] = bpl[(size_t)t * 64];
                    }
#pragma unroll
                    for (int k = 0; k < CTC_ALIGN_PF; ++k) {
                        const int t = g - k;
                        if (t >= t0) {                       // wave-uniform
                            const int mv = (__builtin_amdgcn_readlane((int)w[k], (unsigned)s / NS) >> (2 * ((unsigned)s % NS))) & 3;      // 0 at t = 0
                            if (lane == (t & 63)) { myS = s; myMv = mv; }
                            s = max(s - mv, 0);
                        }
                    }
                }
                const int t = t0 + lane;
                const int up = __shfl_down(myS, 1, 64);
                if (t <= thi) {
                    fr[t] = (myS & 1) ? tg[myS >> 1] : 0;
                    if (myS & 1) {
                        if (myMv != 0 || t == 0) span[myS >> 1] = t;
                        if ((t == thi ? above : up) != myS) span[Lmax + (myS >> 1)] = t;
                    }
                }
                above = __builtin_amdgcn_readfirstlane(myS);
            }
        }
    }
    for (int t = (feasible ? Tb : 0) + lane; t < T; t += 64) fr[t] = -1;
    if (lane == 0) score[b] = sc;
    __syncthreads();
    // ---- spans: one lane per label
    for (int l = lane; l < Lmax; l += 64) {
        const int st = (feasible && l < L) ? span[l] : -1, en = (feasible && l < L) ? span[Lmax + l] : -1;
        if (tok_start) tok_start[(long)b * Lmax + l] = st;
        if (tok_end) tok_end[(long)b * Lmax + l] = en;
        if (tok_logp) {
            float acc = 0.f;
            if (st >= 0) for (int t = st; t <= en; ++t) acc += lp_rows[(long)t * Sp + 2 * l + 1];
            tok_logp[(long)b * Lmax + l] = acc * CTC_LN2;
        }
    }
}

template <int NS, int CH, bool LDS_BP>
__global__ __launch_bounds__(64) void ctc_align_kernel(int T, const int* __restrict__ hlens, const int* __restrict__ targets, int Lmax,
                                                       const int* __restrict__ tlens, int Sp, const float* __restrict__ lp,
                                                       void* __restrict__ bp_ws, int* __restrict__ frames, int* __restrict__ tok_start,
                                                       int* __restrict__ tok_end, float* __restrict__ tok_logp, float* __restrict__ score) {
    typedef typename std::conditional<(NS <= 4), unsigned char, unsigned short>::type BPT;
    extern __shared__ __attribute__((aligned(16))) unsigned char align_sh[];      // back-pointer words (LDS route)
    __shared__ int span[64 * CTC_MAXQ];                                            // 2 * Lmax = Sp - 1 entries
    const int b = blockIdx.x;
    const int Tb = min(hlens[b], T);
    const int L = max(min(tlens[b], Lmax), 0);
    const int* tg = targets + (long)b * Lmax;
    const float* lp_rows = lp + (long)b * T * Sp;
    if (LDS_BP) {
        BPT* bpl = reinterpret_cast<BPT*>(align_sh) + threadIdx.x;
        ctc_align_wave<NS, CH>(bpl, span, b, T, Tb, L, Lmax, Sp, tg, lp_rows, frames, tok_start, tok_end, tok_logp, score);
    } else {
        BPT* bpl = reinterpret_cast<BPT*>(bp_ws) + (size_t)b * T * 64 + threadIdx.x;
        ctc_align_wave<NS, CH>(bpl, span, b, T, Tb, L, Lmax, Sp, tg, lp_rows, frames, tok_start, tok_end, tok_logp, score);
    }
}

// bytes of a back-pointer word (see ctc_align_kernel) and whether T frames of 64 of them go to LDS
static inline size_t ctc_align_word(int Sp) { return Sp <= 256 ? 1 : 2; }
static inline bool ctc_align_in_lds(int T, int Sp) { return (size_t)T * 64 * ctc_align_word(Sp) <= CTC_ALIGN_LDS; }

extern "C" size_t oe_ctc_align_workspace_bytes(int B, int T, int Lmax) {
    if (B <= 0 || T <= 0 || Lmax < 0) return 0;
    const int Sp = 2 * Lmax + 1;
    const size_t lp = ((size_t)B * T * Sp * sizeof(float) + 15) & ~(size_t)15;
    return lp + (ctc_align_in_lds(T, Sp) ? 0 : (size_t)B * T * 64 * ctc_align_word(Sp));
}

extern "C" int oe_ctc_align(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* targets, int Lmax,
                            const int* tlens, int* frames, int* tok_start, int* tok_end, float* tok_logp, float* score,
                            void* workspace, void* stream) {
    OE_REQUIRE(logits && hlens && tlens && frames && score && workspace, "oe_ctc_align: null pointer");
    OE_REQUIRE(targets || Lmax == 0, "oe_ctc_align: null targets");
    OE_REQUIRE(B > 0 && T > 0 && V > 1 && Lmax >= 0 && ldv >= V, "oe_ctc_align: bad shape B=%d T=%d V=%d Lmax=%d ldv=%ld", B, T, V, Lmax, ldv);
    const int Sp = 2 * Lmax + 1;
    OE_REQUIRE(Sp <= 64 * CTC_MAXQ, "oe_ctc_align: target length %d exceeds the 255-label limit of the wave recursion", Lmax);
    hipStream_t st = (hipStream_t)stream;
    float* lp = reinterpret_cast<float*>(workspace);
    void* bp = reinterpret_cast<char*>(workspace) + (((size_t)B * T * Sp * sizeof(float) + 15) & ~(size_t)15);
    ctc_launch_rows(logits, ldv, B, T, V, hlens, targets, Lmax, tlens, Sp, 0.f, nullptr, lp, nullptr, 0, T, st);
    OE_LAUNCH_CHECK("ctc_align_rows");
    const bool in_lds = ctc_align_in_lds(T, Sp);
    const size_t shm = in_lds ? (size_t)T * 64 * ctc_align_word(Sp) : 0;
#define AL(NS, CH, LDS) hipLaunchKernelGGL((ctc_align_kernel<NS, CH, LDS>), dim3(B), dim3(64), shm, st, T, hlens, targets, Lmax, tlens, Sp, lp, bp, \
                                           frames, tok_start, tok_end, tok_logp, score)
#define ALS(NS, CH) do { if (in_lds) AL(NS, CH, true); else AL(NS, CH, false); } while (0)
    if (Sp <= 64) ALS(1, 32); else if (Sp <= 128) ALS(2, 16); else if (Sp <= 256) ALS(4, 8); else ALS(8, 4);
#undef ALS
#undef AL
    OE_LAUNCH_CHECK("ctc_align");
    return 0;
}
