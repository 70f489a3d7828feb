// The CTC alpha / beta recursion with its STATE in float64: shared by the n-best scorer (ctc_nbest.hip) and by the long-launch
// path of the training loss (ctc.hip).  Structure as ctc.hip's float32 k2: log2 domain, a finite "log 0", neighbours by DPP
// shifts, lp prefetched a chunk of frames ahead, the direction a template parameter.  With the state in float64 only the exp /
// log are float32 (bare v_exp_f32 / v_log_f32 on differences in [-inf, 0] and a sum in [1, 3]: ~3e-7 absolute per step whatever
// the magnitude of the state).
#pragma once
#include "oe_common.h"

__device__ __forceinline__ float nb_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float nb_log2(float x) { return __builtin_amdgcn_logf(x); }
#define NB_NEG_D (-1.0e30)
// lane i <- lane i-1 (lane 0 <- NB_NEG_D) / lane i <- lane i+1 (lane 63 <- NB_NEG_D), as two 32-bit DPP moves
template <int CTRL>
__device__ __forceinline__ double nb_shift(double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(NB_NEG_D), __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(NB_NEG_D), __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double nb_shr1(double v) { return nb_shift<0x138>(v); }
__device__ __forceinline__ double nb_shl1(double v) { return nb_shift<0x130>(v); }
// log2(2^a + 2^b + 2^c) + add
__device__ __forceinline__ double nb_lse3_add(double a, double b, double c, float add) {
    const double m = fmax(a, fmax(b, c));
    const float s = nb_exp2((float)(a - m)) + nb_exp2((float)(b - m)) + nb_exp2((float)(c - m));
    return (m + (double)add) + (double)nb_log2(s);
}
// log2(2^a + 2^b) + add: the two-term form (the transducer lattice, rnnt.hip)
__device__ __forceinline__ double nb_lse2_add(double a, double b, double add) {
    const double m = fmax(a, b);
    return (m + add) + (double)nb_log2(1.f + nb_exp2((float)(fmin(a, b) - m)));
}

template <bool FWD, int NS, int CH, bool FULL>
__device__ __forceinline__ void nb_chunk(int c0, int Tb, const long (&ostr)[NS], double (&a)[NS], const double (&cap)[NS],
                                         const float (&cur)[CH][NS], double* (&op)[NS]) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        if (FULL || c0 + i < Tb) {       // wave-uniform; whole chunks carry no test
            const double p1 = FWD ? nb_shr1(a[NS - 1]) : nb_shl1(a[0]);
            const double p2 = FWD ? (NS >= 2 ? nb_shr1(a[NS >= 2 ? NS - 2 : 0]) : nb_shr1(p1))
                                  : (NS >= 2 ? nb_shl1(a[NS >= 2 ? 1 : 0]) : nb_shl1(p1));
            double na[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                double n1, n2;
                if (FWD) {
                    n1 = (j >= 1) ? a[j >= 1 ? j - 1 : 0] : p1;
                    n2 = (j >= 2) ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2);
                } else {
                    n1 = (j + 1 < NS) ? a[j + 1 < NS ? j + 1 : 0] : p1;
                    n2 = (j + 2 < NS) ? a[j + 2 < NS ? j + 2 : 0] : (j + 1 < NS ? p1 : p2);
                }
                na[j] = nb_lse3_add(a[j], n1, fmin(n2, cap[j]), cur[i][j]);
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

// One direction of the recursion over the Tb frames of a row: NS states per lane; CH frames of lp are fetched at a time, one
// chunk ahead.  Every step's column goes to out_rows (Tb, Sp); a[] returns this lane's final values.  tg: the row's tokens,
// read at positions below (S - 1) / 2 only.  dump: one double any lane may scribble on.
template <bool FWD, int NS, int CH>
__device__ __forceinline__ void nb_recurse(int lane, int Tb, int S, int Sp, const int* __restrict__ tg, const float* __restrict__ lp_rows,
                                           double* out_rows, double* dump, double (&a)[NS]) {
    const int s0 = lane * NS;
    double cap[NS];   // upper bound on the s-2 (alpha) / s+2 (beta) term: that transition exists only between different labels
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
        cap[j] = skip ? 3.0e38 : NB_NEG_D;
    }
    // step k of the recursion works on frame  FWD ? k : Tb-1-k
    const long tstride = FWD ? (long)Sp : -(long)Sp;
    const float* lp0 = lp_rows + (long)(FWD ? 0 : Tb - 1) * Sp + s0;
    // states past S store to the dump word with stride 0: the stores of a step need no predicate
    double* op[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) op[j] = valid[j] ? out_rows + (long)(FWD ? 0 : Tb - 1) * Sp + s0 + j : dump;
    long ostr[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) ostr[j] = valid[j] ? tstride : 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int s = s0 + j;
        const bool start = FWD ? (s <= 1) : (s >= S - 2);
        a[j] = NB_NEG_D;
        if (valid[j] && start) a[j] = (double)lp0[j];
        *op[j] = a[j];
    }
    // steps 1 .. Tb-1 in chunks of CH.  States past S carry lp = 0: they stay NB_NEG_D, and their values go to the dump word.
    float cur[CH][NS], nxt[CH][NS];
#pragma unroll
    for (int i = 0; i < CH; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            cur[i][j] = 0.f;
            if (1 + i < Tb && valid[j]) cur[i][j] = lp0[(1 + i) * tstride + j];
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
                if (c0 + CH + i < Tb && valid[j]) nxt[i][j] = lp0[(c0 + CH + i) * tstride + j];
            }
        if (c0 + CH <= Tb) nb_chunk<FWD, NS, CH, true>(c0, Tb, ostr, a, cap, cur, op);
        else nb_chunk<FWD, NS, CH, false>(c0, Tb, ostr, a, cap, cur, op);
        // the next chunk becomes current here: pinning the values makes the compiler wait for the prefetch once per chunk
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                cur[i][j] = nxt[i][j];
                asm volatile("" : "+v"(cur[i][j]));
            }
    }
}
