// CTC prefix scores for the joint CTC/attention beam search, one wavefront per hypothesis and one lane per candidate
// token: psi(g . c), the log-probability that the utterance's label sequence starts with the hypothesis g extended by c,
// and the extended hypothesis' forward state.  Semantics in include/openeat_hip.h; the yardstick is
// tests/ctc_prefix_score_ref.py (the recursion against an enumeration of all alignments).
//
// A wave owns row r = one live hypothesis of utterance r / group.  The parent's state r[t, 0..1] and the blank column
// y[t, blank] are the same for every lane (the row comes from blockIdx alone, so these are uniform loads); what a lane
// owns is its candidate's column y[t, c], a 4-byte gather that depends on nothing the recursion computes.  The chain over
// the frames is three float64 log_adds per frame (n[t, 0], n[t, 1] and psi, independent of each other inside a frame) and
// is latency-bound, so the gathers run CPS_PF frames ahead of it in registers: the next block of frames is requested
// before the current block's chain starts.  phi[t] depends on the parent's state alone and is formed off the chain.
// A frame's candidate states are one 16-byte store per lane, contiguous across the lanes: (r, t, c, 0..1).
// No workspace, no atomics, no LDS, one launch, nothing read on the host: capturable.
//
// log_add is the prefix-beam kernels' (beam.hip): max + log(sum of exp(. - max)) with the maximum's term written down as
// 1 and a -inf term as 0, so two -inf give -inf and never NaN.
#include "oe_common.h"
#include "../../include/openeat_hip.h"

#define CPS_MAXC 64
#define CPS_PF 8                                                // frames of y[t, c] in flight ahead of the chain

__device__ __forceinline__ double cps_neg() { return -__builtin_huge_val(); }
__device__ __forceinline__ double cps_term(double x, double m) { return x == m ? 1.0 : (x == cps_neg() ? 0.0 : exp(x - m)); }
__device__ __forceinline__ double cps_log_add(double a, double b) {
    const double ninf = cps_neg();
    if (a == ninf && b == ninf) return ninf;
    const double m = fmax(a, b);
    return m + log(cps_term(a, m) + cps_term(b, m));
}

// the empty hypothesis' state for R = B * group rows, one lane per row: r[t, 0] = -inf, r[t, 1] = y[0, blank] + .. + y[t, blank]
__global__ __launch_bounds__(64) void ctc_prefix_score_init_kernel(const float* __restrict__ logp, long ldv, const int* __restrict__ lens,
                                                                   int R, int group, int Tmax, int blank, double* __restrict__ state) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int u = r / group;
    const int T = lens ? min(max(lens[u], 0), Tmax) : Tmax;
    const float* y = logp + (size_t)u * Tmax * ldv + blank;
    double2* s = reinterpret_cast<double2*>(state) + (size_t)r * Tmax;
    double acc = 0.0;
    for (int t = 0; t < T; ++t) {
        acc += (double)y[(size_t)t * ldv];
        s[t] = make_double2(cps_neg(), acc);
    }
}

__global__ __launch_bounds__(64) void ctc_prefix_score_kernel(const float* __restrict__ logp, long ldv, const int* __restrict__ lens, int group,
                                                              int Tmax, int V, const double* __restrict__ state_in,
                                                              const int* __restrict__ hyp_len, const int* __restrict__ last_tok,
                                                              const int* __restrict__ cand, int C, int blank, int eos,
                                                              double* __restrict__ psi_out, double* __restrict__ cand_state) {
    const int r = blockIdx.x, lane = threadIdx.x;
    if (lane >= C) return;
    const double NEG = cps_neg();
    const int hl = hyp_len[r];
    if (hl < 0) {                                                // the slot does not exist (wave-uniform): no state is written
        psi_out[(size_t)r * C + lane] = NEG;
        return;
    }
    const int u = r / group;
    const int T = lens ? min(max(lens[u], 0), Tmax) : Tmax;
    const int tok = cand[(size_t)r * C + lane];
    const bool in_range = tok >= 0 && tok < V && tok != blank;
    double psi = NEG;
    if (T == 0) {
        if (in_range && tok == eos && hl == 0) psi = 0.0;
        psi_out[(size_t)r * C + lane] = psi;
        return;
    }
    const double2* rs = reinterpret_cast<const double2*>(state_in) + (size_t)r * Tmax;   // .x non-blank, .y blank
    if (!in_range || tok == eos) {
        if (in_range) { const double2 e = rs[T - 1]; psi = cps_log_add(e.x, e.y); }
        psi_out[(size_t)r * C + lane] = psi;
        return;
    }
    const bool same = hl > 0 && tok == last_tok[r];
    const float* y = logp + (size_t)u * Tmax * ldv;
    const float* yc = y + tok;                                   // this lane's column
    const float* yb = y + blank;
    double2* ns = cand_state ? reinterpret_cast<double2*>(cand_state) + (size_t)r * Tmax * C + lane : nullptr;

    double n0 = hl == 0 ? (double)yc[0] : NEG, n1 = NEG;
    psi = n0;
    if (ns) ns[0] = make_double2(n0, n1);
    float cur[CPS_PF], nxt[CPS_PF];
#pragma unroll
    for (int k = 0; k < CPS_PF; ++k) cur[k] = yc[(size_t)min(1 + k, T - 1) * ldv];
    for (int t0 = 1; t0 < T; t0 += CPS_PF) {
#pragma unroll
        for (int k = 0; k < CPS_PF; ++k) nxt[k] = yc[(size_t)min(t0 + CPS_PF + k, T - 1) * ldv];
#pragma unroll
        for (int k = 0; k < CPS_PF; ++k) {
            const int t = t0 + k;
            if (t < T) {                                         // wave-uniform
                const double2 p = rs[t - 1];
                const double phi = same ? p.y : cps_log_add(p.x, p.y);
                const double yt = (double)cur[k], ybt = (double)yb[(size_t)t * ldv];
                const double m0 = cps_log_add(n0, phi) + yt;
                const double m1 = cps_log_add(n0, n1) + ybt;
                psi = cps_log_add(psi, phi + yt);
                n0 = m0;
                n1 = m1;
                if (ns) ns[(size_t)t * C] = make_double2(n0, n1);
            }
        }
#pragma unroll
        for (int k = 0; k < CPS_PF; ++k) cur[k] = nxt[k];
    }
    psi_out[(size_t)r * C + lane] = psi;
}

static int cps_check_common(const char* who, const float* logp, int B, int Tmax, int V, long ldv, int group, int blank) {
    OE_REQUIRE(B >= 0 && Tmax >= 0 && V >= 1, "%s: bad shape B=%d Tmax=%d V=%d", who, B, Tmax, V);
    OE_REQUIRE(ldv >= V, "%s: leading dimension %ld below V=%d", who, ldv, V);
    OE_REQUIRE(group >= 1, "%s: group must be >= 1 (got %d)", who, group);
    OE_REQUIRE((long)B * group <= 0x7fffffffL, "%s: B=%d x group=%d rows exceed the grid", who, B, group);
    OE_REQUIRE(blank >= 0 && blank < V, "%s: blank=%d outside 0..V-1 (V=%d)", who, blank, V);
    OE_REQUIRE(logp || Tmax == 0, "%s: null pointer (logp)", who);
    return 0;
}

extern "C" int oe_ctc_prefix_score_init(const float* logp, const int* lens, int B, int Tmax, int V, long ldv, int group, int blank,
                                        double* state, void* stream) {
    if (cps_check_common("oe_ctc_prefix_score_init", logp, B, Tmax, V, ldv, group, blank)) return -1;
    OE_REQUIRE(state || Tmax == 0, "oe_ctc_prefix_score_init: null pointer (state)");
    const int R = B * group;
    if (R == 0 || Tmax == 0) return 0;
    hipLaunchKernelGGL(ctc_prefix_score_init_kernel, dim3(oe_cdiv(R, 64)), dim3(64), 0, (hipStream_t)stream, logp, ldv, lens, R, group, Tmax,
                       blank, state);
    OE_LAUNCH_CHECK("ctc_prefix_score_init");
    return 0;
}

extern "C" int oe_ctc_prefix_score(const float* logp, const int* lens, int B, int Tmax, int V, long ldv, int group, const double* state_in,
                                   const int* hyp_len, const int* last_tok, const int* cand, int C, int blank, int eos, double* psi,
                                   double* cand_state, void* stream) {
    if (cps_check_common("oe_ctc_prefix_score", logp, B, Tmax, V, ldv, group, blank)) return -1;
    OE_REQUIRE(C >= 1 && C <= CPS_MAXC, "oe_ctc_prefix_score: C=%d candidates outside 1..%d", C, CPS_MAXC);
    OE_REQUIRE(hyp_len && last_tok && cand && psi, "oe_ctc_prefix_score: null pointer");
    OE_REQUIRE(state_in || Tmax == 0, "oe_ctc_prefix_score: null pointer (state_in)");
    const int R = B * group;
    if (R == 0) return 0;
    hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, logp, ldv, lens, group, Tmax, V, state_in, hyp_len,
                       last_tok, cand, C, blank, eos, psi, cand_state);
    OE_LAUNCH_CHECK("ctc_prefix_score");
    return 0;
}
