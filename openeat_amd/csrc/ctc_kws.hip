// Keyword search over CTC posteriors: where every keyword of a list occurs in every recording, and how confidently.  The
// semantics every layer refers to are in include/openeat_hip.h (oe_ctc_kws); the tie rule is oe_ctc_align's.
//
// A keyword is at most 32 labels, 63 states: one wave holds its trellis column, a state per lane.  What is large is the
// product: K ~ 1000 keywords x T ~ 90 000 frames x V ~ 4000 columns.  Two launches:
//   launch 1  lp_rows_kernel (lp_rows.hip): the blank and the U keyword columns of every frame as lp, a compact row of U + 1 floats.
//   launch 2  kws_kernel: ONE WAVE PER (recording, keyword), KWS_KPW keywords of the same recording per workgroup so that the
//             compact rows their lanes gather share cache lines in the CU's L1.  Lane s-1 holds state s: its value v and the
//             frame st at which its path entered state 1.  v and st reach lane+1 by one wave shift (kws_shr1, as seg_shr1) and
//             lane+2 by a second one; the lane's lp of KWS_PF frames is loaded a chunk ahead of the recursion, so the serial
//             chain of a frame is the shifts, three compares and an add, never a memory latency.  The lane of state 2L-1
//             runs the candidate / pending-hit scan inside the same loop (float64 cross-multiplied comparisons; exact: a
//             float32 times an integer below 2^21) and writes a hit when it is emitted.  The start frame is carried, so
//             there is no back-pointer table, no back-trace and no (B,K,T) array.
//             Bound: a latency chain of Tb steps per wave; the waves of all (b,k) run side by side.  Measured (T = 90 000,
//             K = 1000, V = 4233): the float64 scan on every frame 19.7 ms with 8 frames ahead and 18.7 ms with 32
//             (100 VGPRs; the chain was not waiting on memory); behind a float32 filter, 16 frames ahead, 14.7 ms.
// No waves wait for each other, no LDS, no atomics, no allocation, no host read: capturable.
#include <stdlib.h>
#include "oe_common.h"
#include "../../include/openeat_hip.h"

#define KWS_NEG (-1.0e30f)          // finite "log 0" (see ctc.hip): KWS_NEG + lp stays KWS_NEG in fp32
#define KWS_MAX_T (1 << 20)
#define KWS_MAX_K 65535
#define KWS_MAX_L 32
#define KWS_KPW 4                   // keywords (waves) per workgroup of launch 2
#define KWS_PF 16                   // frames of lp in flight ahead of the recursion

// lane i <- lane i-1, lane 0 <- fill (row shift right by one across the whole wave)
__device__ __forceinline__ float kws_shr1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, KWS_NEG), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int kws_shr1(int v) { return __builtin_amdgcn_update_dpp(-1, v, 0x138, 0xf, 0xf, false); }

// ---------------------------------------------------------------- launch 2 ----
struct KwsParams {
    const float* cw; int T, U, K, Lmax, max_hits;
    const int* hlens; const int* kw_col; const int* klens; const float* thr;
    int* n_hits; int* hit_start; int* hit_end; float* hit_score;
    int* best_start; int* best_end; float* best_score;
};

__global__ __launch_bounds__(64 * KWS_KPW) void kws_kernel(const KwsParams p) {
    const int lane = threadIdx.x & 63;
    const int nkb = (p.K + KWS_KPW - 1) / KWS_KPW;
    const int b = blockIdx.x / nkb;
    const int k = (blockIdx.x % nkb) * KWS_KPW + (threadIdx.x >> 6);
    if (k >= p.K) return;                                                    // whole waves; nothing below is a workgroup barrier
    const int T = p.T, U = p.U, max_hits = p.max_hits;
    const int Tb = max(min(p.hlens[b], T), 0);
    const int L = max(min(p.klens[k], p.Lmax), 0);
    const int ns = 2 * L - 1;                                                // states, lanes 0 .. ns-1
    const long bk = (long)b * p.K + k;
    int* hs = p.hit_start + bk * max_hits;
    int* he = p.hit_end + bk * max_hits;
    float* hv = p.hit_score + bk * max_hits;

    // the scan's state: meaningful on the lane of state 2L-1 only
    int count = 0;
    bool pend = false, has_best = false;
    int p_st = -1, p_en = -1, b_st = -1, b_en = -1;
    float p_sc = 0.f, b_sc = -INFINITY, b_nf = 1.f;                           // b_nf: the best's frames as a float

    if (L > 0 && Tb > 0) {
        const int* kc = p.kw_col + (long)k * p.Lmax;
        const int s = lane + 1;
        const bool live = lane < ns, lab = live && (s & 1);
        int ci = 0;                                                          // the lane's column of a compact row: 0 = blank
        bool skip = false;
        if (lab) {
            const int u = min(max(kc[s >> 1], 0), U - 1);
            ci = 1 + u;
            skip = s >= 3 && u != min(max(kc[(s >> 1) - 1], 0), U - 1);
        }
        const bool endl = lane == ns - 1;
        const float thr_f = p.thr[k];
        const double thr = (double)thr_f;
        const long rw = U + 1;
        const float* base = p.cw + (long)b * T * rw + ci;
        float v = KWS_NEG;
        int st = -1;
        float cur[KWS_PF], nxt[KWS_PF];
#pragma unroll
        for (int i = 0; i < KWS_PF; ++i) cur[i] = base[(long)min(i, Tb - 1) * rw];   // clamped: always a row launch 1 wrote
        for (int c0 = 0; c0 < Tb; c0 += KWS_PF) {
#pragma unroll
            for (int i = 0; i < KWS_PF; ++i) nxt[i] = base[(long)min(c0 + KWS_PF + i, Tb - 1) * rw];
#pragma unroll
            for (int i = 0; i < KWS_PF; ++i) {
                const int t = c0 + i;
                if (t < Tb) {                                                // uniform over the wave
                    const float v1 = kws_shr1(v);
                    const int s1 = kws_shr1(st);
                    const float v2 = kws_shr1(v1);
                    const int s2 = kws_shr1(s1);
                    // a candidate replaces the best only if strictly greater, in the order stay, step, skip, fresh
                    float best = v;
                    int bs = st;
                    if (v1 > best) { best = v1; bs = s1; }
                    if (skip && v2 > best) { best = v2; bs = s2; }
                    if (lane == 0 && 0.f > best) { best = 0.f; bs = t; }
                    v = live ? best + cur[i] : KWS_NEG;
                    st = bs;
                    // state 2L-1 reachable: a candidate.  It changes nothing unless it beats the best or passes the threshold, and
                    // nearly none does: both are first asked in float32 with a margin of 2e-6 (a product of a float32 and an
                    // integer below 2^24 is within 2^-24 of exact), and only what may pass goes on to the exact float64 comparisons.
                    const float nf = (float)(t - st + 1);
                    const float lim_b = b_sc * nf, lim_t = thr_f * nf;
                    const bool may = v * b_nf >= lim_b - fabsf(lim_b) * 2e-6f || v >= lim_t - fabsf(lim_t) * 2e-6f;
                    if (endl && v > 0.5f * KWS_NEG && may) {
                        const int n = t - st + 1;
                        const double sc = (double)v;
                        if (!has_best || sc * (double)(b_en - b_st + 1) > (double)b_sc * (double)n) {
                            has_best = true; b_st = st; b_en = t; b_sc = v; b_nf = nf;
                        }
                        if (sc >= thr * (double)n) {
                            if (pend && st <= p_en) {
                                if (sc * (double)(p_en - p_st + 1) > (double)p_sc * (double)n) { p_st = st; p_en = t; p_sc = v; }
                            } else {
                                if (pend) {
                                    if (count < max_hits) { hs[count] = p_st; he[count] = p_en; hv[count] = p_sc; }
                                    ++count;
                                }
                                pend = true; p_st = st; p_en = t; p_sc = v;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < KWS_PF; ++i) {
                cur[i] = nxt[i];
                asm volatile("" : "+v"(cur[i]));
            }
        }
        if (endl && pend) {
            if (count < max_hits) { hs[count] = p_st; he[count] = p_en; hv[count] = p_sc; }
            ++count;
        }
        // the scan's results -> every lane
        const int src = ns - 1;
        count = __shfl(count, src, 64);
        b_st = __shfl(b_st, src, 64);
        b_en = __shfl(b_en, src, 64);
        b_sc = __shfl(b_sc, src, 64);
    }
    for (int i = min(count, max_hits) + lane; i < max_hits; i += 64) {
        hs[i] = -1;
        he[i] = -1;
        hv[i] = 0.f;
    }
    if (lane == 0) {
        p.n_hits[bk] = count;
        if (p.best_start) p.best_start[bk] = b_st;
        if (p.best_end) p.best_end[bk] = b_en;
        if (p.best_score) p.best_score[bk] = b_sc;
    }
}

// ---------------------------------------------------------------- host -------
extern "C" size_t oe_ctc_kws_workspace_bytes(int B, int T, int U) {
    if (B <= 0 || T <= 0 || T > KWS_MAX_T || U <= 0) return 0;
    return (size_t)B * (size_t)T * ((size_t)U + 1) * sizeof(float);
}

extern "C" int oe_ctc_kws(const oe_ctc_kws_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_kws: null args");
    const oe_ctc_kws_args& a = *args;
    OE_REQUIRE(a.kws, "oe_ctc_kws: null kws (the keyword set)");
    const oe_keyword_set& q = *a.kws;
    OE_REQUIRE(a.logits, "oe_ctc_kws: null logits");
    OE_REQUIRE(a.hlens, "oe_ctc_kws: null hlens");
    OE_REQUIRE(a.n_hits && a.hit_start && a.hit_end && a.hit_score, "oe_ctc_kws: null output (n_hits, hit_start, hit_end, hit_score)");
    OE_REQUIRE(a.workspace, "oe_ctc_kws: null workspace");
    OE_REQUIRE(a.B > 0 && a.T > 0 && a.T <= KWS_MAX_T && a.V > 1 && a.ldv >= a.V,
               "oe_ctc_kws: bad shape B=%d T=%d V=%d ldv=%ld (1 <= B, 1 <= T <= 2^20, ldv >= V)", a.B, a.T, a.V, a.ldv);
    OE_REQUIRE(q.K >= 1 && q.K <= KWS_MAX_K, "oe_ctc_kws: K=%d keywords outside 1 .. %d", q.K, KWS_MAX_K);
    OE_REQUIRE(q.Lmax >= 1 && q.Lmax <= KWS_MAX_L, "oe_ctc_kws: Lmax=%d outside 1 .. %d labels, a state per lane of a wave", q.Lmax, KWS_MAX_L);
    OE_REQUIRE(q.U >= 1 && q.U < a.V, "oe_ctc_kws: U=%d distinct tokens outside 1 .. V-1 = %d", q.U, a.V - 1);
    OE_REQUIRE(q.cols && q.kw_col && q.klens && q.thr, "oe_ctc_kws: null table in kws (cols, kw_col, klens, thr)");
    OE_REQUIRE(a.max_hits >= 1, "oe_ctc_kws: max_hits=%d < 1", a.max_hits);
    OE_REQUIRE((((uintptr_t)a.workspace) & 15) == 0, "oe_ctc_kws: workspace must be 16-byte aligned");
    const long nkb = (q.K + KWS_KPW - 1) / KWS_KPW;
    OE_REQUIRE((long)a.B * nkb <= 0x7fffffffL, "oe_ctc_kws: B=%d x K=%d exceeds one launch's workgroups", a.B, q.K);
    hipStream_t st = (hipStream_t)stream;
    float* cw = reinterpret_cast<float*>(a.workspace);
    if (int rc = oe_lp_rows("oe_ctc_kws", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, q.cols, q.U, a.normalized, cw, nullptr, st))
        return rc;
    KwsParams p;
    p.cw = cw; p.T = a.T; p.U = q.U; p.K = q.K; p.Lmax = q.Lmax; p.max_hits = a.max_hits;
    p.hlens = a.hlens; p.kw_col = q.kw_col; p.klens = q.klens; p.thr = q.thr;
    p.n_hits = a.n_hits; p.hit_start = a.hit_start; p.hit_end = a.hit_end; p.hit_score = a.hit_score;
    p.best_start = a.best_start; p.best_end = a.best_end; p.best_score = a.best_score;
    hipLaunchKernelGGL(kws_kernel, dim3((unsigned)(a.B * nkb)), dim3(64 * KWS_KPW), 0, st, p);
    OE_LAUNCH_CHECK("ctc_kws");
    return 0;
}
