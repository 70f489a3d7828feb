// Grouped CTC forward-backward: the exact CTC log-likelihood of each of `group` hypotheses of an utterance (an n-best list)
// and the gradient of a weighted sum of them with respect to the utterance's logits - the device half of minimum word error
// rate training (utils/mwer.py, ASRModel.forward_mwer).  The specification is the comment of oe_ctc_nbest_score in
// include/openeat_hip.h; the yardstick is tests/ctc_nbest_ref.py.
//
// The expanded form - the logits repeated `group` times through oe_ctc_loss_fused - reads and writes the logits group-fold
// although all hypotheses of an utterance read the same rows.  Here the logits are read once per pass, whatever the group:
//   score  k1 rows      : one wave per frame (b, t) reads the row ONCE: (max, 1 / sum exp) and the log2-probabilities at the
//                         2L+1 states of each of the utterance's hypotheses -> lp (R, T, Sp).  B*T*V*4 bytes.
//          k2 alphabeta : one block per row r: wave 0 runs alpha, wave 1 beta (only when `saved` is asked for); the recursion
//                         is ctc.hip's (log2 domain, finite "log 0", neighbours by DPP shifts, lp prefetched a chunk ahead)
//                         with the state in float64 (see k2).
//                         Then the block's eight waves turn alpha + beta into occupancies, a frame each: the blank's (a fixed-order
//                         reduction over the even states) and one per DISTINCT label of the hypothesis (the states of a label
//                         that occurs more than once are summed along a chain, first occurrence first).  Latency-bound: R lone
//                         chains of Tb steps.
//   grad   k3 grad      : one workgroup per dlogits row: -G_b * softmax into LDS (G_b = sum of g over the feasible rows, slot
//                         ascending), then g[r] * occ added at the blank and label columns by one wave, slot after slot - within
//                         a slot the columns are distinct, so the lanes work side by side; across slots the order is the
//                         program's - and the row is stored once.  One read of the logits, one write of dlogits.
// No atomics on floats anywhere; every sum has a fixed order: bit-identical from run to run.
#include "oe_common.h"
#include "ctc_f64.h"
#include "../../include/openeat_hip.h"

#define NB_NEG_INF (-INFINITY)
#define NB_MAXQ 8                 // states per lane (Sp <= 64 * 8)
#define NB_LOG2E 1.4426950408889634f
#define NB_AB_THREADS 512         // k2 with `saved`: waves 0 / 1 run alpha / beta, all eight share the occupancy frames
#define NB_MAX_GROUP 64
#define NB_MAX_L 255

// ------------------------------------------------------------------ k1 ------
// NV4 > 0: the row is NV4 float4 per lane, held in registers (V <= 256 * NV4, rows 16-byte aligned); NV4 == 0: any V and
// alignment, the row is read twice (the second time from cache).
template <int NV4>
__global__ __launch_bounds__(256) void ctc_nbest_rows_kernel(const float* __restrict__ logits, long ldv, long rows, int T, int V,
                                                              const int* __restrict__ hlens, const int* __restrict__ hyps, long hyp_ld,
                                                              const int* __restrict__ hyp_lens, int group, int Lmax, int Sp,
                                                              float* __restrict__ lp_out, float2* __restrict__ rowstat) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (int)(row / T), t = (int)(row % T);
    if (t >= min(hlens[b], T)) return;                  // padded frame: nothing reads its lp or statistics
    const float* p = logits + row * ldv;
    float m = NB_NEG_INF, s = 0.f;
    if (NV4 > 0) {
        const int nv = (V + 3) >> 2;
        float4 v[NV4 > 0 ? NV4 : 1];
        const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int i = lane + 64 * j;
            v[j] = make_float4(NB_NEG_INF, NB_NEG_INF, NB_NEG_INF, NB_NEG_INF);
            if (i < nv) v[j] = p4[i];
            const int e = i * 4;                          // columns past V (row padding) do not count
            if (e + 1 >= V) v[j].y = NB_NEG_INF;
            if (e + 2 >= V) v[j].z = NB_NEG_INF;
            if (e + 3 >= V) v[j].w = NB_NEG_INF;
        }
#pragma unroll
        for (int j = 0; j < NV4; ++j) m = fmaxf(m, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
        m = wave_max(m);
#pragma unroll
        for (int j = 0; j < NV4; ++j) s += (__expf(v[j].x - m) + __expf(v[j].y - m)) + (__expf(v[j].z - m) + __expf(v[j].w - m));
    } else {
        for (int i = lane; i < V; i += 64) m = fmaxf(m, p[i]);
        m = wave_max(m);
        for (int i = lane; i < V; i += 64) s += __expf(p[i] - m);
    }
    s = wave_sum(s);
    const float l2s = __builtin_amdgcn_logf(s);
    if (lane == 0) rowstat[row] = make_float2(m, 1.f / s);
    // log2-probabilities at the states of every hypothesis of this utterance (the row is in cache now).  A token outside
    // 0 .. V-1 is never an index: its row is infeasible and its lp is not read.
    const int nel = group * Sp;
    for (int idx = lane; idx < nel; idx += 64) {
        const int n = idx / Sp, st = idx - n * Sp;
        const long r = (long)b * group + n;
        const int L = hyp_lens[r];
        if (L < 0 || L > Lmax || st > 2 * L) continue;
        const int c = (st & 1) ? hyps[r * hyp_ld + (st >> 1)] : 0;
        const float x = (c >= 0 && c < V) ? p[c] : 0.f;
        lp_out[(r * T + t) * Sp + st] = (x - m) * NB_LOG2E - l2s;
    }
}

// ------------------------------------------------------------------ k2 ------
// The recursion has the structure of ctc.hip's k2 (copied, so that file's compiled code does not change: log2 domain, a finite
// "log 0", neighbours by DPP shifts, lp prefetched a chunk of frames ahead, the direction a template parameter), but the STATE
// is float64.  An n-best list is scored with tolerances on every hypothesis' occupancies, 2^(alpha + beta - lp - ll): in
// float32 a column that has drifted to -1800 (300 frames of a 140-token hypothesis) takes 1e-4 of rounding per step, and
// the occupancies missed their tolerance by 3x (measured); keeping the columns near zero by subtracting a lagged maximum
// still missed it by 5x at 520 frames x 255 tokens, because the states that matter lie far below their column's maximum.
// With the state in float64 only the exp / log are float32 (bare v_exp_f32 / v_log_f32 on differences in [-inf, 0] and a
// sum in [1, 3]: ~3e-7 absolute per step whatever the magnitude of the state).
// (nb_recurse and its helpers: ctc_f64.h, shared with the long-launch path of ctc.hip)

// One block per row.  occ == nullptr: alpha only (the score; two waves).  Otherwise beta runs beside alpha on wave 1, then
// all eight waves share the frames of the occupancy pass (a frame costs a dependent global-memory round trip: on two waves
// that pass took longer than the recursion), and the block leaves in `saved`:  cls (R, Lp) - entry 0 is the blank's class 0, entry 1 + i the token at position i if that is the first
// occurrence of its class in the hypothesis, else -1 (as is everything behind the length);  occ (R, T, Lp) - at the entries
// whose cls >= 0 and the frames below Tb, the posterior probability that the alignment emits that class at that frame.
// alpha / beta are written and read back inside the block: not __restrict__, not const.
template <int NS, int CH>
__global__ __launch_bounds__(NB_AB_THREADS) void ctc_nbest_alphabeta_kernel(int T, int V, int group, const int* __restrict__ hlens,
                                                                   const int* __restrict__ hyps, long hyp_ld, const int* __restrict__ hyp_lens,
                                                                   int Lmax, int Sp, const float* __restrict__ lp, double* alpha, double* beta,
                                                                   float* __restrict__ logp, float* __restrict__ occ, int* __restrict__ cls,
                                                                   double* __restrict__ dump) {
    __shared__ double fin[2];
    __shared__ int flaw[2];                    // adjacent equal tokens; any token outside 1 .. V-1
    __shared__ int link[NB_MAX_L + 1];            // position i: (next position with the same token, + 1; 0 = none) | first << 16
    __shared__ float gam[NB_AB_THREADS / 64][64 * NB_MAXQ];
    const int r = blockIdx.x, b = r / group;
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;     // 128 threads without `saved`, NB_AB_THREADS with
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Tb = min(hlens[b], T);
    const int L = hyp_lens[r];
    const int* tg = hyps + (long)r * hyp_ld;
    if (tid < 2) { fin[tid] = NB_NEG_D; flaw[tid] = 0; }
    __syncthreads();
    const bool shape_ok = L >= 0 && L <= Lmax && Tb > 0;       // block-uniform
    if (shape_ok) {
        int rep = 0, oob = 0;
        for (int i = tid; i < L; i += nthr) {
            const int c = tg[i];
            if (c < 1 || c >= V) oob = 1;
            if (i > 0 && tg[i - 1] == c) ++rep;
        }
        if (rep) atomicAdd(&flaw[0], rep);
        if (oob) atomicOr(&flaw[1], 1);
    }
    __syncthreads();
    if (!shape_ok || flaw[1] || Tb < L + flaw[0]) {
        if (tid == 0) logp[r] = NB_NEG_INF;
        return;
    }
    const int S = 2 * L + 1, Lp = Lmax + 1;
    if (occ) {
        for (int i = tid; i < L; i += nthr) {
            const int c = tg[i];
            int head = 1, nx = 0;
            for (int q = 0; q < i; ++q) if (tg[q] == c) { head = 0; break; }
            for (int q = i + 1; q < L; ++q) if (tg[q] == c) { nx = q + 1; break; }
            link[i] = nx | (head << 16);
            cls[(long)r * Lp + 1 + i] = head ? c : -1;
        }
        for (int j = L + 1 + tid; j < Lp; j += nthr) cls[(long)r * Lp + j] = -1;
        if (tid == 0) cls[(long)r * Lp] = 0;
    }
    const long base = (long)r * T * Sp;
    {
        double a[NS];
        if (wv == 0) {
            nb_recurse<true, NS, CH>(lane, Tb, S, Sp, tg, lp + base, alpha + base, dump, a);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if (lane * NS + j == S - 1) fin[0] = a[j];
                if (lane * NS + j == S - 2) fin[1] = a[j];
            }
        } else if (wv == 1 && occ) {
            nb_recurse<false, NS, CH>(lane, Tb, S, Sp, tg, lp + base, beta + base, dump, a);
        }
    }
    __syncthreads();
    // log2-likelihood from the last column's two end states; a value that still carries the NB_NEG_D scale means no
    // alignment exists (the test above already excludes that; this is the recursion's own word on it)
    const double f0 = fin[0], f1 = fin[1];
    const double fm = fmax(f0, f1);
    const double ll = fm + (double)nb_log2(nb_exp2((float)(f0 - fm)) + nb_exp2((float)(f1 - fm)));
    const bool feasible = ll > 0.5 * NB_NEG_D;
    if (tid == 0) logp[r] = feasible ? (float)(ll * 0.69314718055994530942) : NB_NEG_INF;
    if (!occ || !feasible) return;
    // occupancies, one wave per frame: 2^(alpha + beta - lp - ll), the exponent formed in float64
    float* gm = gam[wv];
    for (int t = wv; t < Tb; t += nthr >> 6) {
        const long o = base + (long)t * Sp;
        float blank = 0.f;
        for (int s = lane; s < S; s += 64) {
            const float v = nb_exp2((float)(alpha[o + s] + beta[o + s] - (double)lp[o + s] - ll));
            gm[s] = v;
            if (!(s & 1)) blank += v;
        }
        blank = wave_sum(blank);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        float* orow = occ + ((long)r * T + t) * Lp;
        if (lane == 0) orow[0] = blank;
        for (int i = lane; i < L; i += 64) {
            const int info = link[i];
            if (info >> 16) {
                float v = gm[2 * i + 1];
                for (int nx = (info & 0xffff) - 1; nx >= 0; nx = (link[nx] & 0xffff) - 1) v += gm[2 * nx + 1];
                orow[1 + i] = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------ k3 ------
// One workgroup per dlogits row.  The row passes through LDS in pieces of NBG_CW columns (one piece up to 4096 columns); the
// sparse terms of up to NBG_STAGE / Lp slots at a time are fetched by the whole block into LDS (class, value), then wave 0
// adds them slot after slot.  Within a slot the classes are distinct (cls keeps a label's first occurrence only), so the lanes
// of the wave touch different words; a wave's LDS operations execute in program order, so a later slot sees an earlier one's sums.
#define NBG_CW 4096
#define NBG_STAGE 1024
template <bool VEC>
__global__ __launch_bounds__(256) void ctc_nbest_grad_kernel(const float* __restrict__ logits, long ldv, int T, int V,
                                                              const int* __restrict__ hlens, int group, int Lp,
                                                              const float* __restrict__ logp, const float* __restrict__ g,
                                                              const float* __restrict__ occ, const int* __restrict__ cls,
                                                              const float2* __restrict__ rowstat, float* __restrict__ dlogits) {
    __shared__ __attribute__((aligned(16))) float rowbuf[NBG_CW];
    __shared__ float sval[NBG_STAGE];
    __shared__ int scls[NBG_STAGE];
    const long row = blockIdx.x;
    const int b = (int)(row / T), t = (int)(row % T);
    const int tid = threadIdx.x;
    const float* p = logits + row * ldv;
    float* d = dlogits + row * ldv;
    if (t >= min(hlens[b], T)) {                                  // padded frame: exact zeros in the V columns
        for (int i = tid; i < V; i += 256) d[i] = 0.f;
        return;
    }
    float G = 0.f;
    for (int n = 0; n < group; ++n) {
        const int r = b * group + n;
        if (logp[r] != NB_NEG_INF) G += g[r];                     // g of an infeasible row is not read into anything
    }
    const float2 st = rowstat[row];
    const float f = G * st.y;
    const int nslot = NBG_STAGE / Lp;                             // >= 4: Lp <= 256
    for (int c0 = 0; c0 < V; c0 += NBG_CW) {
        const int cw = min(NBG_CW, V - c0);
        const int nv = VEC ? (cw >> 2) : 0;
        if (VEC) {
            const float4* p4 = reinterpret_cast<const float4*>(p + c0);
            for (int i = tid; i < nv; i += 256) {
                const float4 x = p4[i];
                reinterpret_cast<float4*>(rowbuf)[i] = make_float4(0.f - f * __expf(x.x - st.x), 0.f - f * __expf(x.y - st.x),
                                                                   0.f - f * __expf(x.z - st.x), 0.f - f * __expf(x.w - st.x));
            }
        }
        for (int i = 4 * nv + tid; i < cw; i += 256) rowbuf[i] = 0.f - f * __expf(p[c0 + i] - st.x);
        __syncthreads();
        for (int n0 = 0; n0 < group; n0 += nslot) {
            const int nb = min(nslot, group - n0);
            for (int e = tid; e < nb * Lp; e += 256) {
                const int k = e / Lp, j = e - k * Lp;
                const long r = (long)b * group + n0 + k;
                int c = -1;
                float v = 0.f;
                if (logp[r] != NB_NEG_INF) {
                    c = cls[r * Lp + j];
                    if (c >= c0 && c < c0 + cw) v = g[r] * occ[(r * T + t) * Lp + j];
                    else c = -1;
                }
                scls[e] = c;
                sval[e] = v;
            }
            __syncthreads();
            if (tid < 64) {
                for (int k = 0; k < nb; ++k) {
                    for (int j = tid; j < Lp; j += 64) {
                        const int c = scls[k * Lp + j];
                        if (c >= 0) rowbuf[c - c0] += sval[k * Lp + j];
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            __syncthreads();
        }
        if (VEC) {
            float4* d4 = reinterpret_cast<float4*>(d + c0);
            for (int i = tid; i < nv; i += 256) d4[i] = reinterpret_cast<const float4*>(rowbuf)[i];
        }
        for (int i = 4 * nv + tid; i < cw; i += 256) d[c0 + i] = rowbuf[i];
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host ------
static inline size_t nb_up16(size_t x) { return (x + 15) & ~(size_t)15; }
struct NbLayout {                                  // byte offsets
    size_t ws_stat, ws_lp, ws_alpha, ws_beta, ws_dump, ws_total;
    size_t sv_occ, sv_cls, sv_stat, sv_total;
};
static NbLayout nb_layout(int B, int T, int group, int Lmax) {
    NbLayout l;
    const size_t R = (size_t)B * group, Sp = 2 * (size_t)Lmax + 1, Lp = (size_t)Lmax + 1, rows = (size_t)B * T;
    const size_t trellis = nb_up16(R * T * Sp * sizeof(float));      // lp: float32; alpha, beta: float64
    l.ws_stat = 0;
    l.ws_lp = nb_up16(rows * sizeof(float2));
    l.ws_alpha = l.ws_lp + trellis;
    l.ws_beta = l.ws_alpha + 2 * trellis;
    l.ws_dump = l.ws_beta + 2 * trellis;
    l.ws_total = l.ws_dump + 64;
    l.sv_occ = 0;
    l.sv_cls = nb_up16(R * T * Lp * sizeof(float));
    l.sv_stat = l.sv_cls + nb_up16(R * Lp * sizeof(int));
    l.sv_total = l.sv_stat + nb_up16(rows * sizeof(float2));
    return l;
}
static bool nb_dims_ok(int B, int T, int group, int Lmax) {
    return B > 0 && T > 0 && group >= 1 && group <= NB_MAX_GROUP && Lmax >= 0 && Lmax <= NB_MAX_L;
}
extern "C" size_t oe_ctc_nbest_workspace_bytes(int B, int T, int group, int Lmax) {
    return nb_dims_ok(B, T, group, Lmax) ? nb_layout(B, T, group, Lmax).ws_total : 0;
}
extern "C" size_t oe_ctc_nbest_saved_bytes(int B, int T, int group, int Lmax) {
    return nb_dims_ok(B, T, group, Lmax) ? nb_layout(B, T, group, Lmax).sv_total : 0;
}

static int nb_check(const char* who, const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* hyps, long hyp_ld,
                    const int* hyp_lens, int group, int Lmax) {
    OE_REQUIRE(logits && hlens && hyp_lens, "%s: null pointer", who);
    OE_REQUIRE(hyps || Lmax == 0, "%s: null hyps", who);
    OE_REQUIRE(B > 0 && T > 0 && V > 1, "%s: bad shape B=%d T=%d V=%d", who, B, T, V);
    OE_REQUIRE(group >= 1 && group <= NB_MAX_GROUP, "%s: group must be 1 .. %d (got %d)", who, NB_MAX_GROUP, group);
    OE_REQUIRE(Lmax >= 0 && Lmax <= NB_MAX_L, "%s: Lmax must be 0 .. %d (got %d)", who, NB_MAX_L, Lmax);
    OE_REQUIRE(ldv >= V, "%s: leading dimension ldv=%ld below V=%d", who, ldv, V);
    OE_REQUIRE(hyp_ld >= Lmax, "%s: leading dimension hyp_ld=%ld below Lmax=%d", who, hyp_ld, Lmax);
    return 0;
}

extern "C" int oe_ctc_nbest_score(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* hyps, long hyp_ld,
                                  const int* hyp_lens, int group, int Lmax, float* logp, void* saved, void* workspace, void* stream) {
    if (int rc = nb_check("oe_ctc_nbest_score", logits, ldv, B, T, V, hlens, hyps, hyp_ld, hyp_lens, group, Lmax)) return rc;
    OE_REQUIRE(logp && workspace, "oe_ctc_nbest_score: null pointer (logp / workspace)");
    OE_REQUIRE((((uintptr_t)workspace) & 15) == 0 && (((uintptr_t)saved) & 15) == 0, "oe_ctc_nbest_score: workspace / saved must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const NbLayout l = nb_layout(B, T, group, Lmax);
    char* ws = static_cast<char*>(workspace);
    char* sv = static_cast<char*>(saved);
    float2* rowstat = reinterpret_cast<float2*>(sv ? sv + l.sv_stat : ws + l.ws_stat);
    float* lp = reinterpret_cast<float*>(ws + l.ws_lp);
    double* alpha = reinterpret_cast<double*>(ws + l.ws_alpha);
    double* beta = reinterpret_cast<double*>(ws + l.ws_beta);
    double* dump = reinterpret_cast<double*>(ws + l.ws_dump);
    float* occ = sv ? reinterpret_cast<float*>(sv + l.sv_occ) : nullptr;
    int* cls = sv ? reinterpret_cast<int*>(sv + l.sv_cls) : nullptr;
    const int Sp = 2 * Lmax + 1, R = B * group;
    const long rows = (long)B * T;
    const bool vec = (((uintptr_t)logits) & 15) == 0 && ldv % 4 == 0 && ldv >= (((long)V + 3) & ~3L);
#define ROWS(NV4) hipLaunchKernelGGL((ctc_nbest_rows_kernel<NV4>), dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, logits, ldv, rows, T, V, hlens, \
                                     hyps, hyp_ld, hyp_lens, group, Lmax, Sp, lp, rowstat)
    if (vec && V <= 256 * 4) ROWS(4); else if (vec && V <= 256 * 16) ROWS(16); else ROWS(0);
#undef ROWS
    OE_LAUNCH_CHECK("ctc_nbest_rows");
#define AB(NS, CH) hipLaunchKernelGGL((ctc_nbest_alphabeta_kernel<NS, CH>), dim3(R), dim3(occ ? NB_AB_THREADS : 128), 0, st, T, V, group, hlens, hyps, hyp_ld, \
                                      hyp_lens, Lmax, Sp, lp, alpha, beta, logp, occ, cls, dump)
    if (Sp <= 64) AB(1, 32); else if (Sp <= 128) AB(2, 16); else if (Sp <= 256) AB(4, 8); else AB(8, 4);
#undef AB
    OE_LAUNCH_CHECK("ctc_nbest_alphabeta");
    return 0;
}

extern "C" int oe_ctc_nbest_grad(const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* hyps, long hyp_ld,
                                 const int* hyp_lens, int group, int Lmax, const float* logp, const float* g, const void* saved,
                                 float* dlogits, void* workspace, void* stream) {
    (void)workspace;
    if (int rc = nb_check("oe_ctc_nbest_grad", logits, ldv, B, T, V, hlens, hyps, hyp_ld, hyp_lens, group, Lmax)) return rc;
    OE_REQUIRE(logp && g && saved && dlogits, "oe_ctc_nbest_grad: null pointer (logp / g / saved / dlogits)");
    OE_REQUIRE(dlogits != logits, "oe_ctc_nbest_grad: dlogits may not alias logits");
    OE_REQUIRE((((uintptr_t)saved) & 15) == 0, "oe_ctc_nbest_grad: saved must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const NbLayout l = nb_layout(B, T, group, Lmax);
    const char* sv = static_cast<const char*>(saved);
    const float* occ = reinterpret_cast<const float*>(sv + l.sv_occ);
    const int* cls = reinterpret_cast<const int*>(sv + l.sv_cls);
    const float2* rowstat = reinterpret_cast<const float2*>(sv + l.sv_stat);
    const bool vec = (((uintptr_t)logits) & 15) == 0 && (((uintptr_t)dlogits) & 15) == 0 && ldv % 4 == 0;
    const long rows = (long)B * T;
    OE_REQUIRE(rows <= 0x7fffffffL, "oe_ctc_nbest_grad: B * T = %ld rows exceed the grid limit", rows);
    if (vec) hipLaunchKernelGGL((ctc_nbest_grad_kernel<true>), dim3((unsigned)rows), dim3(256), 0, st, logits, ldv, T, V, hlens, group, Lmax + 1,
                                logp, g, occ, cls, rowstat, dlogits);
    else hipLaunchKernelGGL((ctc_nbest_grad_kernel<false>), dim3((unsigned)rows), dim3(256), 0, st, logits, ldv, T, V, hlens, group, Lmax + 1,
                            logp, g, occ, cls, rowstat, dlogits);
    OE_LAUNCH_CHECK("ctc_nbest_grad");
    return 0;
}
