// Beam-pruned graph CTC likelihood and its gradient over large token graphs: oe_ctc_graph_logp's sum by oe_ctc_graph_beam's token
// passing.  The semantics every layer refers to are in include/openeat_hip.h (oe_ctc_graph_beam_logp).
//
//   launch 1  lp_rows_kernel (lp_rows.hip): lp as a compact row of U + 1 floats; for the gradient also the row's log-sum-exp.
//   launch 2  bl_kernel: ONE WORKGROUP of 1024 threads PER UTTERANCE, the state in global memory as float64 in the log2 domain
//             (ctc_graph_logp.hip's numbers), guarded by stamps and active lists (ctc_graph_beam.hip's machinery: a stamp s says
//             "alive as input of frame s - 1", lists are appended to through an LDS counter, positions are in no fixed order).
//   launch 3  bl_dense_kernel (gradient): a wave per dlogits row: g * (occ - softmax).
// A sum pushed to a node by many threads must not depend on the order of arrival, and float atomics are out.  So a sum over a
// list is a maximum (order-free) and then a sum of 64-bit FIXED-POINT integers, exp2(value - maximum) at scale 2^40, by integer
// atomicAdd: associative, hence order-free; at most 2^22 terms of at most 2^41 each cannot overflow.
// Frame t of the forward sweep over L_t, the states alive as input of frame t; a barrier behind each step:
//   1  every entry touches a node (itself, or its arc's dst; the first toucher appends it to the touched list); an arc pushes
//      (its value rounded to float32, inverted id) to key1[dst] by a 64-bit atomicMax: id1, and v1 = the float64 value of id1.
//      v1 is the maximum up to a float32 rounding, which is all a reference point has to be.
//   2  every arc whose label is not that of id1 pushes to key2[dst]: id2 / v2.
//   3  every arc adds exp2(v - v1) to S1[dst] and, if its label is not c1 = label(id1), to G[its in-group at dst] and
//      exp2(v - v2) to S2[dst].
//   3a per touched node: tot = LSE(n_{t-1}[q], v1 + log2 S1) and x2 = LSE(n_{t-1}[q], v2 + log2 S2), kept by position in the
//      touched list with v1, S1, c1; keys and sums are reset here; n_t[q] = lp[t,0] + tot is a candidate.
//   3b the arcs leaving the touched nodes (a thread per node, a wave per node of more than 16 leaving arcs): "the node and every
//      incoming arc of another label" is x2 if the arc's label is c1, else LSE(n_{t-1}[q], v1 + log2(S1 - G[in_xg[a]])): an exact
//      integer difference that always contains id1's 2^40, so never a cancellation.
//   4  the arcs of L_t that 3b did not reach stay; every arc of L_t resets its G slot.
//   5  best_t by a workgroup maximum; thr_t = best_t - beam.
//   6  the candidates at or above thr_t are appended to L_{t+1} (the gradient keeps their ids and alpha per frame).
// Work per frame: O(|L_t| + the arcs leaving the touched nodes); a hub's in-arcs are never walked.  logZ: the maximum over the
// last list, then the fixed-point sum.  The gradient's backward sweep is the mirror image: the arcs of S_{t+1} push
// w + lp + beta to the aggregates of their src (out-groups), the entries of S_t pull; the new betas go to a list-ordered
// buffer and are committed behind a barrier.  Occupancies add as fixed-point integers into a row of U + 1 per frame.
// Values written by an atomic are read by atomic loads; everything else is written and read by the waves of one workgroup with
// a barrier between.  No workgroup waits for another, no float atomics, no allocation, no host read.
#include <stdlib.h>
#include "ctc_graph_common.h"
#include "ctc_f64.h"
#include "../../include/openeat_hip.h"

#define BL_BLOCK 1024
#define BL_WAVES (BL_BLOCK / 64)
#define BL_MAX_T GRAPH_MAX_T
#define BL_MAX_Q OE_CTC_GRAPH_BEAM_MAX_NODES
#define BL_MAX_A OE_CTC_GRAPH_BEAM_MAX_ARCS
#define BL_WIDE 16                                // a node of more leaving arcs than this takes a wave, not a thread
#define BL_NEG (-1.0e30)                          // "log 0"
#define BL_DEAD (-5.0e29)                         // a value at or below this is unreachable
#define BL_LOG2E 1.4426950408889634
#define BL_LN2 0.6931471805599453
#define BL_FIX 1099511627776.f                    // 2^40

// ---------------------------------------------------------------- numbers ----
// log2(2^a + 2^b): commutative bit for bit, exact (= the other) against "log 0"
__device__ __forceinline__ double bl_lse(double a, double b) {
    const double m = fmax(a, b);
    return m + (double)nb_log2(1.f + nb_exp2((float)(fmin(a, b) - m)));
}
// a product into the log2 domain, pinned so that no instantiation fuses it into a neighbouring sum
__device__ __forceinline__ double bl_scale(float x) {
    double v = (double)x * BL_LOG2E;
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ double bl_lp(float x) { return bl_scale(fmaxf(x, -1.0e30f)); }
// 2^d at scale 2^40, d <= 0 up to a rounding (held to 1)
__device__ __forceinline__ beam_u64 bl_fix(double d) { return (beam_u64)(nb_exp2(fminf((float)d, 1.f)) * BL_FIX); }
// log2(S / 2^40), S > 0: the exponent exactly, the top 24 bits through v_log_f32
__device__ __forceinline__ double bl_log2fix(beam_u64 S) {
    const int lz = __clzll((long long)S);
    const float m = (float)(unsigned)((S << lz) >> 40) * (1.f / 8388608.f);
    return (double)(23 - lz) + (double)nb_log2(m);
}
__device__ __forceinline__ beam_u64 bl_shfl_xor_u64(beam_u64 v, int o) {
    const int lo = __shfl_xor((int)(unsigned)v, o, 64), hi = __shfl_xor((int)(unsigned)(v >> 32), o, 64);
    return ((beam_u64)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ beam_u64 bl_wave_sum_u64(beam_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += bl_shfl_xor_u64(v, o);
    return v;
}
__device__ __forceinline__ double bl_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, oe_shfl_xor_f64(v, o));
    return v;
}
__device__ __forceinline__ void bl_add(beam_u64* p, beam_u64 v) { atomicAdd(p, v); }

// ---------------------------------------------------------------- launch 2 ----
// The per-utterance workspace: byte offsets of its parts, every one a multiple of 16 (Q, A, M are rounded up to 4).
struct BlLayout {
    size_t key1, key2, s1, s2, grp, rs, ns, tstamp, bns, brs, zero_bytes;     // key1 .. brs: zeroed before frame 0
    size_t nv, rv, nb, rb, cand, touched, wide, tnp, tv1, ts1, tx2, ttot, tc1, tb, cnt, ids, alpha, bytes;
    long Mp;
};
static BlLayout bl_layout(bool grad, long T, long Q, long A, long M) {
    const size_t Qp = (size_t)(Q + 3) & ~(size_t)3, Ap = (size_t)(A + 3) & ~(size_t)3, Mp = (size_t)(M + 3) & ~(size_t)3;
    const size_t Tp = (size_t)(T + 3) & ~(size_t)3;
    BlLayout l;
    size_t o = 0;
    l.key1 = o; o += 8 * Qp;
    l.key2 = o; o += 8 * Qp;
    l.s1 = o; o += 8 * Qp;
    l.s2 = o; o += 8 * Qp;
    l.grp = o; o += 8 * Ap;
    l.rs = o; o += 4 * Ap;
    l.ns = o; o += 4 * Qp;
    l.tstamp = o; o += 4 * Qp;
    l.bns = o; o += grad ? 4 * Qp : 0;
    l.brs = o; o += grad ? 4 * Ap : 0;
    l.zero_bytes = o;
    l.nv = o; o += 8 * Qp;
    l.rv = o; o += 8 * Ap;
    l.nb = o; o += grad ? 8 * Qp : 0;
    l.rb = o; o += grad ? 8 * Ap : 0;
    l.cand = o; o += 4 * (Qp + Ap);
    l.touched = o; o += 4 * Mp;
    l.wide = o; o += 4 * Mp;
    l.tnp = o; o += 8 * Mp;
    l.tv1 = o; o += 8 * Mp;
    l.ts1 = o; o += 8 * Mp;
    l.tx2 = o; o += 8 * Mp;
    l.ttot = o; o += 8 * Mp;
    l.tc1 = o; o += 4 * Mp;
    l.tb = o; o += grad ? 8 * Mp : 0;
    l.cnt = o; o += grad ? 4 * Tp : 0;
    l.ids = o; o += grad ? 4 * (size_t)T * Mp : 8 * Mp;                       // the score: two lists, in turn
    l.alpha = o; o += grad ? 8 * (size_t)T * Mp : 0;
    l.bytes = o;                              // score 52 Q' + 24 A' + 60 M';  gradient 64 Q' + 36 A' + 60 M' + 4 T' + 12 T M'
    l.Mp = (long)Mp;
    return l;
}

struct BlParams {
    const float* cw; char* ws; BlLayout l;
    int T, U, Q, A, M, max_active;
    double beam2;                                                             // the beam in the log2 domain
    const int* hlens; const int* src; const int* dst; const int* col; const float* w; const float* fin;
    const int* out_ptr; const int* out_arc; const int* in_grp; const int* in_xg; const int* out_grp; const int* out_xg;
    float* logp; int* status; int* peak; double* logz; beam_u64* occ;
};

template <bool GRAD>
__global__ __launch_bounds__(BL_BLOCK) void bl_kernel(const BlParams p) {
    __shared__ int s_ntouched, s_nwide, s_ncand, s_nsurv;
    __shared__ double red_d[BL_WAVES];
    __shared__ beam_u64 red_u[BL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int T = p.T, U = p.U, Q = p.Q, A = p.A, M = p.M;
    const int QA = Q + A;
    const long Mp = p.l.Mp;
    char* ws = p.ws + (size_t)b * p.l.bytes;
    beam_u64* key1 = reinterpret_cast<beam_u64*>(ws + p.l.key1);
    beam_u64* key2 = reinterpret_cast<beam_u64*>(ws + p.l.key2);
    beam_u64* s1 = reinterpret_cast<beam_u64*>(ws + p.l.s1);
    beam_u64* s2 = reinterpret_cast<beam_u64*>(ws + p.l.s2);
    beam_u64* grp = reinterpret_cast<beam_u64*>(ws + p.l.grp);
    int* rs = reinterpret_cast<int*>(ws + p.l.rs);
    int* ns = reinterpret_cast<int*>(ws + p.l.ns);
    int* tstamp = reinterpret_cast<int*>(ws + p.l.tstamp);
    double* nv = reinterpret_cast<double*>(ws + p.l.nv);
    double* rv = reinterpret_cast<double*>(ws + p.l.rv);
    int* cand = reinterpret_cast<int*>(ws + p.l.cand);
    int* touched = reinterpret_cast<int*>(ws + p.l.touched);
    int* wide = reinterpret_cast<int*>(ws + p.l.wide);
    double* tnp = reinterpret_cast<double*>(ws + p.l.tnp);
    double* tv1 = reinterpret_cast<double*>(ws + p.l.tv1);
    beam_u64* ts1 = reinterpret_cast<beam_u64*>(ws + p.l.ts1);
    double* tx2 = reinterpret_cast<double*>(ws + p.l.tx2);
    double* ttot = reinterpret_cast<double*>(ws + p.l.ttot);
    int* tc1 = reinterpret_cast<int*>(ws + p.l.tc1);
    int* ids = reinterpret_cast<int*>(ws + p.l.ids);
    double* alpha = reinterpret_cast<double*>(ws + p.l.alpha);
    int* cntv = reinterpret_cast<int*>(ws + p.l.cnt);
    const int Tb = max(min(p.hlens[b], T), 0);
    const long rw = U + 1;
    const float* cw = p.cw + (long)b * T * rw;
    beam_u64* occ = GRAD ? p.occ + (long)b * T * rw : nullptr;
    auto col_of = [&](int a) { return min(max(p.col[a], 0), U - 1); };
    auto dst_of = [&](int a) { return min(max(p.dst[a], 0), Q - 1); };
    auto src_of = [&](int a) { return min(max(p.src[a], 0), Q - 1); };
    auto state_of = [&](int c) { return min(max(c, 0), QA - 1); };
    auto arc_id = [&](beam_u64 k) { return min(max(beam_key_id(k), 0), A - 1); };
    auto fin2 = [&](int q) { return fmax(bl_scale(p.fin[q]), BL_NEG); };
    auto list_of = [&](int t) { return GRAD ? ids + (size_t)t * Mp : ids + (size_t)(t & 1) * Mp; };   // S_t = L_{t+1}

    // ---- before frame 0: the one sweep over the graph's size; n[0] = 0 is alive as input of frame 0
    {
        int4* z = reinterpret_cast<int4*>(ws);
        const size_t nz = p.l.zero_bytes / 16;
        for (size_t i = tid; i < nz; i += BL_BLOCK) z[i] = make_int4(0, 0, 0, 0);
    }
    if (GRAD)
        for (long i = tid; i < (long)Tb * rw; i += BL_BLOCK) occ[i] = 0;
    if (tid == 0) { s_ntouched = 0; s_nwide = 0; s_ncand = 0; s_nsurv = 0; }
    __syncthreads();
    if (tid == 0) { nv[0] = 0.0; ns[0] = 1; }
    __syncthreads();

    int n = Tb > 0 ? 1 : 0;                                                  // |L_t|
    int peak = 0, status = OE_CTC_GRAPH_BEAM_OK, done = 0;
    for (int t = 0; t < Tb; ++t) {
        const int* Lin = list_of(max(t - 1, 0));                              // L_t (t >= 1); L_0 = {node 0} is not stored
        int* Lout = list_of(t);
        const int tag_in = t + 1, tag_out = t + 2;
        const float* row = cw + (long)t * rw;
        const double lp0 = bl_lp(row[0]);
        double lmax = -INFINITY;

        // ---- 1: touch, push v1
        for (int base = 0; base < n; base += BL_BLOCK) {
            const int i = base + tid;
            bool first = false;
            int d = 0;
            if (i < n) {
                const int c = t ? state_of(Lin[i]) : 0;
                if (c < Q) d = c;
                else {
                    const int a = c - Q;
                    d = dst_of(a);
                    atomicMax(&key1[d], beam_key((float)rv[a], a));
                }
                first = atomicMax(&tstamp[d], tag_in) != tag_in;
            }
            const int j = beam_append(&s_ntouched, first);
            if (first && j < M) touched[j] = d;
        }
        __syncthreads();
        if (tid == 0) { s_ncand = 0; s_nsurv = 0; }

        // ---- 2: push v2, the best of a label other than id1's
        for (int i = tid; i < n; i += BL_BLOCK) {
            const int c = t ? state_of(Lin[i]) : 0;
            if (c < Q) continue;
            const int a = c - Q, d = dst_of(a);
            const int id1 = arc_id(beam_load(&key1[d]));
            if (col_of(a) != col_of(id1)) atomicMax(&key2[d], beam_key((float)rv[a], a));
        }
        __syncthreads();

        // ---- 3: the fixed-point sums
        for (int i = tid; i < n; i += BL_BLOCK) {
            const int c = t ? state_of(Lin[i]) : 0;
            if (c < Q) continue;
            const int a = c - Q, d = dst_of(a);
            const int id1 = arc_id(beam_load(&key1[d]));
            const double va = rv[a];
            const beam_u64 e1 = bl_fix(va - rv[id1]);
            bl_add(&s1[d], e1);
            if (col_of(a) != col_of(id1)) {
                bl_add(&grp[min(max(p.in_grp[a], 0), A - 1)], e1);
                const int id2 = arc_id(beam_load(&key2[d]));
                bl_add(&s2[d], bl_fix(va - rv[id2]));
            }
        }
        __syncthreads();

        // ---- 3a: per touched node its aggregates; the node's own new value
        const int nt = min(s_ntouched, M);
        for (int base = 0; base < nt; base += BL_BLOCK) {
            const int j = base + tid;
            bool made = false, is_wide = false;
            int q = 0;
            if (j < nt) {
                q = min(max(touched[j], 0), Q - 1);
                const beam_u64 k1 = beam_load(&key1[q]), k2 = beam_load(&key2[q]);
                const beam_u64 S1 = beam_load(&s1[q]), S2 = beam_load(&s2[q]);
                const bool alive = ns[q] == tag_in;
                const double np = alive ? nv[q] : BL_NEG;                     // n_{t-1}[q]
                double v1 = BL_NEG, tot = np, x2 = np;
                int c1 = -1;
                if (k1) {
                    beam_clear(&key1[q]);
                    beam_clear(&s1[q]);
                    const int id1 = arc_id(k1);
                    v1 = rv[id1];
                    c1 = col_of(id1);
                    if (S1) tot = bl_lse(np, v1 + bl_log2fix(S1));
                }
                if (k2) {
                    beam_clear(&key2[q]);
                    beam_clear(&s2[q]);
                    if (S2) x2 = bl_lse(np, rv[arc_id(k2)] + bl_log2fix(S2));
                }
                tnp[j] = np; tv1[j] = v1; ts1[j] = k1 ? S1 : 0; tx2[j] = x2; ttot[j] = tot; tc1[j] = c1;
                const double nn = lp0 + tot;
                if (nn > BL_DEAD) {
                    nv[q] = nn;
                    ns[q] = tag_out;
                    lmax = fmax(lmax, nn);
                    made = true;
                }
                const int lo = min(max(p.out_ptr[q], 0), A), hi = min(max(p.out_ptr[q + 1], lo), A);
                is_wide = hi - lo > BL_WIDE;
            }
            const int ci = beam_append(&s_ncand, made);
            if (made && ci < QA) cand[ci] = q;
            const int wi = beam_append(&s_nwide, is_wide);
            if (is_wide && wi < M) wide[wi] = j;
        }
        __syncthreads();

        // ---- 3b: the arcs leaving the touched nodes
        auto make_arc = [&](bool has, int a, int j) {
            bool made = false;
            if (has) {
                const int k = col_of(a);
                double X;
                if (k == tc1[j]) X = tx2[j];
                else {
                    const int x = min(max(p.in_xg[a], -1), A - 1);
                    const beam_u64 G = x >= 0 ? beam_load(&grp[x]) : 0, S1 = ts1[j];
                    X = G == 0 ? ttot[j] : S1 > G ? bl_lse(tnp[j], tv1[j] + bl_log2fix(S1 - G)) : tnp[j];
                }
                const double stay = rs[a] == tag_in ? rv[a] : BL_NEG;
                const double v = bl_lp(row[1 + k]) + bl_lse(stay, bl_scale(p.w[a]) + X);
                if (v > BL_DEAD) {
                    rv[a] = v;
                    rs[a] = tag_out;
                    lmax = fmax(lmax, v);
                    made = true;
                }
            }
            const int ci = beam_append(&s_ncand, made);
            if (made && ci < QA) cand[ci] = Q + a;
        };
        for (int base = 0; base < nt; base += BL_BLOCK) {
            const int j = base + tid;
            int lo = 0, deg = 0;
            if (j < nt) {
                const int q = min(max(touched[j], 0), Q - 1);
                lo = min(max(p.out_ptr[q], 0), A);
                deg = min(max(p.out_ptr[q + 1], lo), A) - lo;
                if (deg > BL_WIDE) deg = 0;                                   // a wave's, below
            }
            for (int e = 0; e < BL_WIDE; ++e) {
                const bool has = e < deg;
                if (__ballot(has) == 0) break;                                // the same for the whole wave
                make_arc(has, has ? min(max(p.out_arc[lo + e], 0), A - 1) : 0, j);
            }
        }
        const int nw = min(s_nwide, M);
        for (int i = wave; i < nw; i += BL_WAVES) {
            const int j = min(max(wide[i], 0), nt - 1);
            const int q = min(max(touched[j], 0), Q - 1);
            const int lo = min(max(p.out_ptr[q], 0), A), deg = min(max(p.out_ptr[q + 1], lo), A) - lo;
            for (int e0 = 0; e0 < deg; e0 += 64) {
                const bool has = e0 + lane < deg;
                make_arc(has, has ? min(max(p.out_arc[lo + e0 + lane], 0), A - 1) : 0, j);
            }
        }
        __syncthreads();
        if (tid == 0) { s_ntouched = 0; s_nwide = 0; }

        // ---- 4: the arcs of L_t whose src has no alive state: stay.  Every arc of L_t resets its group's sum.
        for (int base = 0; base < n; base += BL_BLOCK) {
            const int i = base + tid;
            bool made = false;
            int a = 0;
            if (i < n) {
                const int c = t ? state_of(Lin[i]) : 0;
                if (c >= Q) {
                    a = c - Q;
                    beam_clear(&grp[min(max(p.in_grp[a], 0), A - 1)]);
                    if (rs[a] == tag_in) {
                        const double v = bl_lp(row[1 + col_of(a)]) + rv[a];
                        if (v > BL_DEAD) {
                            rv[a] = v;
                            rs[a] = tag_out;
                            lmax = fmax(lmax, v);
                            made = true;
                        }
                    }
                }
            }
            const int ci = beam_append(&s_ncand, made);
            if (made && ci < QA) cand[ci] = Q + a;
        }

        // ---- 5: best_t, thr_t
        lmax = bl_wave_max(lmax);
        if (lane == 0) red_d[wave] = lmax;
        __syncthreads();
        double best = red_d[0];
#pragma unroll
        for (int i = 1; i < BL_WAVES; ++i) best = fmax(best, red_d[i]);
        const double thr = t < Tb - 1 ? best - p.beam2 : -INFINITY;

        // ---- 6: prune; the survivors are L_{t+1}
        const int nc = min(s_ncand, QA);
        double* aout = GRAD ? alpha + (size_t)t * Mp : nullptr;
        for (int base = 0; base < nc; base += BL_BLOCK) {
            const int i = base + tid;
            bool keep = false;
            int c = 0;
            double v = 0.0;
            if (i < nc) {
                c = state_of(cand[i]);
                v = c < Q ? nv[c] : rv[c - Q];
                keep = !(v < thr);
                if (!keep) { if (c < Q) ns[c] = 0; else rs[c - Q] = 0; }
            }
            const int si = beam_append(&s_nsurv, keep);
            if (keep && si < M) {
                Lout[si] = c;
                if (GRAD) aout[si] = v;
            }
        }
        __syncthreads();
        const int cnt = s_nsurv;
        peak = max(peak, cnt);
        if (cnt > p.max_active) { status = OE_CTC_GRAPH_BEAM_OVERFLOW; peak = cnt; break; }
        if (GRAD && tid == 0) cntv[t] = cnt;
        n = cnt;
        if (cnt == 0) break;
        done = t + 1;
    }

    // ---- logZ over the last list: the maximum, then the fixed-point sum (neither depends on the list's order)
    const bool whole = Tb > 0 && done == Tb;
    const int* Llast = list_of(max(Tb - 1, 0));
    auto end_value = [&](int i) {
        const int c = state_of(Llast[i]);
        return c < Q ? nv[c] + fin2(c) : rv[c - Q] + fin2(dst_of(c - Q));
    };
    double zm = -INFINITY;
    if (whole)
        for (int i = tid; i < n; i += BL_BLOCK) zm = fmax(zm, end_value(i));
    zm = bl_wave_max(zm);
    __syncthreads();                                                          // red_d was read in the last frame
    if (lane == 0) red_d[wave] = zm;
    __syncthreads();
    zm = red_d[0];
#pragma unroll
    for (int i = 1; i < BL_WAVES; ++i) zm = fmax(zm, red_d[i]);
    const bool ok = whole && zm > BL_DEAD;
    beam_u64 zs = 0;
    if (ok)
        for (int i = tid; i < n; i += BL_BLOCK) zs += bl_fix(end_value(i) - zm);
    zs = bl_wave_sum_u64(zs);
    if (lane == 0) red_u[wave] = zs;
    __syncthreads();
    zs = red_u[0];
#pragma unroll
    for (int i = 1; i < BL_WAVES; ++i) zs += red_u[i];
    const double z = ok && zs ? zm + bl_log2fix(zs) : BL_NEG;
    if (tid == 0) {
        if (p.logp) p.logp[b] = ok ? (float)(z * BL_LN2) : -INFINITY;
        if (p.status) p.status[b] = status == OE_CTC_GRAPH_BEAM_OVERFLOW ? status : ok ? OE_CTC_GRAPH_BEAM_OK : OE_CTC_GRAPH_BEAM_INFEASIBLE;
        if (p.peak) p.peak[b] = peak;
        if (GRAD) p.logz[b] = ok ? z : BL_NEG;
    }
    if (!GRAD || !ok) return;

    // ---- beta on the sub-lattice and the occupancies.  nb / rb hold beta of the frame their stamp names (stamp t + 1: frame t).
    int* bns = reinterpret_cast<int*>(ws + p.l.bns);
    int* brs = reinterpret_cast<int*>(ws + p.l.brs);
    double* nb = reinterpret_cast<double*>(ws + p.l.nb);
    double* rb = reinterpret_cast<double*>(ws + p.l.rb);
    double* tb = reinterpret_cast<double*>(ws + p.l.tb);
    __syncthreads();
    for (int t = Tb - 1; t >= 0; --t) {
        const int* Lt = list_of(t);
        const int nt = min(max(cntv[t], 0), M);
        const double* al = alpha + (size_t)t * Mp;
        const bool last = t == Tb - 1;
        const int* Ln = list_of(min(t + 1, Tb - 1));                          // S_{t+1}
        const int nn = last ? 0 : min(max(cntv[t + 1], 0), M);
        const float* row = cw + (long)min(t + 1, Tb - 1) * rw;                // beta_t reads lp of frame t + 1
        const double lp0 = bl_lp(row[0]);
        const int tag_next = t + 2;
        auto y_of = [&](int a) { return (bl_scale(p.w[a]) + bl_lp(row[1 + col_of(a)])) + rb[a]; };   // enter a at frame t + 1
        // ---- b1 .. b3: the arcs of S_{t+1} push to their src
        for (int i = tid; i < nn; i += BL_BLOCK) {
            const int c = state_of(Ln[i]);
            if (c < Q) continue;
            const int a = c - Q;
            atomicMax(&key1[src_of(a)], beam_key((float)y_of(a), a));
        }
        __syncthreads();
        for (int i = tid; i < nn; i += BL_BLOCK) {
            const int c = state_of(Ln[i]);
            if (c < Q) continue;
            const int a = c - Q, s = src_of(a);
            if (col_of(a) != col_of(arc_id(beam_load(&key1[s])))) atomicMax(&key2[s], beam_key((float)y_of(a), a));
        }
        __syncthreads();
        for (int i = tid; i < nn; i += BL_BLOCK) {
            const int c = state_of(Ln[i]);
            if (c < Q) continue;
            const int a = c - Q, s = src_of(a);
            const int id1 = arc_id(beam_load(&key1[s]));
            const double ya = y_of(a);
            const beam_u64 e1 = bl_fix(ya - y_of(id1));
            bl_add(&s1[s], e1);
            if (col_of(a) != col_of(id1)) {
                bl_add(&grp[min(max(p.out_grp[a], 0), A - 1)], e1);
                bl_add(&s2[s], bl_fix(ya - y_of(arc_id(beam_load(&key2[s])))));
            }
        }
        __syncthreads();
        // ---- b4: the entries of S_t pull; their occupancies
        for (int base = 0; base < nt; base += BL_BLOCK) {
            const int i = base + tid;
            beam_u64 o_node = 0;
            if (i < nt) {
                const int c = state_of(Lt[i]);
                double beta;
                if (last) beta = c < Q ? fin2(c) : fin2(dst_of(c - Q));
                else if (c < Q) {
                    beta = bns[c] == tag_next ? lp0 + nb[c] : BL_NEG;
                    const beam_u64 k1 = beam_load(&key1[c]), S1 = beam_load(&s1[c]);
                    if (k1 && S1) beta = bl_lse(beta, y_of(arc_id(k1)) + bl_log2fix(S1));
                } else {
                    const int a = c - Q, d = dst_of(a), k = col_of(a);
                    beta = brs[a] == tag_next ? bl_lp(row[1 + k]) + rb[a] : BL_NEG;
                    beta = bl_lse(beta, bns[d] == tag_next ? lp0 + nb[d] : BL_NEG);
                    const beam_u64 k1 = beam_load(&key1[d]);
                    if (k1) {
                        const int id1 = arc_id(k1);
                        double X = BL_NEG;
                        if (k == col_of(id1)) {
                            const beam_u64 k2 = beam_load(&key2[d]), S2 = beam_load(&s2[d]);
                            if (k2 && S2) X = y_of(arc_id(k2)) + bl_log2fix(S2);
                        } else {
                            const int x = min(max(p.out_xg[a], -1), A - 1);
                            const beam_u64 G = x >= 0 ? beam_load(&grp[x]) : 0, S1 = beam_load(&s1[d]);
                            if (S1 > G) X = y_of(id1) + bl_log2fix(S1 - G);
                        }
                        beta = bl_lse(beta, X);
                    }
                }
                beta = fmax(beta, BL_NEG);
                tb[i] = beta;
                const beam_u64 o = bl_fix(al[i] + beta - z);
                if (c < Q) o_node = o;
                else if (o) bl_add(&occ[(long)t * rw + 1 + col_of(c - Q)], o);
            }
            o_node = bl_wave_sum_u64(o_node);                                 // the blank's column: one add per wave
            if (lane == 0 && o_node) bl_add(&occ[(long)t * rw], o_node);
        }
        __syncthreads();
        // ---- b5: reset the aggregates by walking S_{t+1}; commit beta_t
        for (int i = tid; i < nn; i += BL_BLOCK) {
            const int c = state_of(Ln[i]);
            if (c < Q) continue;
            const int a = c - Q, s = src_of(a);
            beam_clear(&key1[s]); beam_clear(&key2[s]); beam_clear(&s1[s]); beam_clear(&s2[s]);
            beam_clear(&grp[min(max(p.out_grp[a], 0), A - 1)]);
        }
        for (int i = tid; i < nt; i += BL_BLOCK) {
            const int c = state_of(Lt[i]);
            if (c < Q) { nb[c] = tb[i]; bns[c] = t + 1; }
            else { rb[c - Q] = tb[i]; brs[c - Q] = t + 1; }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- launch 3 ----
// One wave per dlogits row.
__global__ __launch_bounds__(256) void bl_dense_kernel(const float* __restrict__ logits, long ldv, long rows, int T, int V,
                                                        const int* __restrict__ hlens, const float* __restrict__ g,
                                                        const double* __restrict__ logz, const float* __restrict__ lse,
                                                        const beam_u64* __restrict__ occ, int U, const int* __restrict__ inv, int n_inv,
                                                        float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (int)(row / T), t = (int)(row % T);
    float* dl = dlogits + row * ldv;
    if (t >= hlens[b] || !(logz[b] > BL_DEAD)) {                              // g of an infeasible utterance is not read
        for (int v = lane; v < V; v += 64) dl[v] = 0.f;
        return;
    }
    const float gb = g[b], c = lse[row];
    const float* x = logits + row * ldv;
    const beam_u64* oc = occ + row * (long)(U + 1);
    for (int v = lane; v < V; v += 64) {
        const int k = v < n_inv ? min(inv[v], U) : -1;
        const float o = k >= 0 ? (float)oc[k] * (1.f / BL_FIX) : 0.f;
        dl[v] = gb * (o - expf(x[v] - c));
    }
}

// ---------------------------------------------------------------- host -------
static bool bl_shape_ok(long B, long T, long U, long Q, long A, long max_active) {
    return B > 0 && T > 0 && T <= BL_MAX_T && U > 0 && Q >= 1 && Q <= BL_MAX_Q && A >= 1 && A <= BL_MAX_A && max_active >= 1;
}
static size_t bl_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t bl_rows_bytes(long B, long T, long U) { return bl_up16((size_t)B * (size_t)T * ((size_t)U + 1) * 4); }
static long bl_capacity(long Q, long A, long max_active) { return max_active < Q + A ? max_active : Q + A; }

extern "C" size_t oe_ctc_graph_beam_logp_workspace_bytes(int B, int T, int U, int Q, int A, int max_active) {
    if (!bl_shape_ok(B, T, U, Q, A, max_active)) return 0;
    return bl_rows_bytes(B, T, U) + (size_t)B * bl_layout(false, T, Q, A, bl_capacity(Q, A, max_active)).bytes;
}

extern "C" size_t oe_ctc_graph_beam_logp_grad_workspace_bytes(int B, int T, int U, int Q, int A, int max_active) {
    if (!bl_shape_ok(B, T, U, Q, A, max_active)) return 0;
    return 3 * bl_rows_bytes(B, T, U) + bl_up16((size_t)B * (size_t)T * 4) + bl_up16((size_t)B * 8) +
           (size_t)B * bl_layout(true, T, Q, A, bl_capacity(Q, A, max_active)).bytes;
}

// the checks the two entries share; everything is reported before any launch
static int bl_check(const char* name, const oe_beam_logp_graph* graph, const float* logits, long ldv, int B, int T, int V, const int* hlens,
                    const void* workspace, int max_active, float beam, const int* status, const int* peak) {
    if (int rc = graph_check(name, graph, logits, ldv, B, T, V, hlens, workspace, nullptr)) return rc;
    const oe_beam_logp_graph& g = *graph;
    OE_REQUIRE(status && peak, "%s: null output (status, peak)", name);
    OE_REQUIRE(g.Q >= 1 && g.Q <= BL_MAX_Q, "%s: Q=%d nodes outside 1 .. %d", name, g.Q, BL_MAX_Q);
    OE_REQUIRE(g.A >= 1 && g.A <= BL_MAX_A, "%s: A=%d arcs outside 1 .. %d", name, g.A, BL_MAX_A);
    OE_REQUIRE(g.n_inv >= 0, "%s: n_inv=%d < 0", name, g.n_inv);
    OE_REQUIRE(g.in_ptr && g.src && g.dst && g.label && g.col && g.w && g.final && g.cols && g.out_ptr && g.out_arc && g.in_grp &&
                   g.in_xg && g.out_grp && g.out_xg && (g.inv || g.n_inv == 0),
               "%s: null table in graph (in_ptr, src, dst, label, col, w, final, cols, out_ptr, out_arc, in_grp, in_xg, out_grp, out_xg, inv)",
               name);
    OE_REQUIRE(max_active >= 1, "%s: max_active=%d < 1", name, max_active);
    OE_REQUIRE(beam >= 0.f, "%s: beam=%g is not >= 0 (+inf: no pruning)", name, (double)beam);
    return 0;
}

static BlParams bl_params(bool grad, const oe_beam_logp_graph& g, const float* cw, char* ws, int T, const int* hlens, int max_active,
                          float beam) {
    BlParams p;
    p.cw = cw; p.ws = ws;
    p.M = (int)bl_capacity(g.Q, g.A, max_active);
    p.l = bl_layout(grad, T, g.Q, g.A, p.M);
    p.T = T; p.U = g.U; p.Q = g.Q; p.A = g.A; p.max_active = max_active;
    p.beam2 = (double)beam * BL_LOG2E;
    p.hlens = hlens; p.src = g.src; p.dst = g.dst; p.col = g.col; p.w = g.w; p.fin = g.final;
    p.out_ptr = g.out_ptr; p.out_arc = g.out_arc; p.in_grp = g.in_grp; p.in_xg = g.in_xg; p.out_grp = g.out_grp; p.out_xg = g.out_xg;
    p.logp = nullptr; p.status = nullptr; p.peak = nullptr; p.logz = nullptr; p.occ = nullptr;
    return p;
}

extern "C" int oe_ctc_graph_beam_logp(const oe_ctc_graph_beam_logp_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph_beam_logp: null args");
    const oe_ctc_graph_beam_logp_args& a = *args;
    if (int rc = bl_check("oe_ctc_graph_beam_logp", a.graph, a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.workspace, a.max_active, a.beam,
                          a.status, a.peak))
        return rc;
    OE_REQUIRE(a.logp, "oe_ctc_graph_beam_logp: null logp");
    const oe_beam_logp_graph& g = *a.graph;
    hipStream_t st = (hipStream_t)stream;
    float* cw = reinterpret_cast<float*>(a.workspace);
    if (int rc = oe_lp_rows("oe_ctc_graph_beam_logp", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, g.cols, g.U, a.normalized, cw, nullptr, st))
        return rc;
    BlParams p = bl_params(false, g, cw, reinterpret_cast<char*>(a.workspace) + bl_rows_bytes(a.B, a.T, g.U), a.T, a.hlens, a.max_active,
                           a.beam);
    p.logp = a.logp; p.status = a.status; p.peak = a.peak;
    hipLaunchKernelGGL(bl_kernel<false>, dim3((unsigned)a.B), dim3(BL_BLOCK), 0, st, p);
    OE_LAUNCH_CHECK("ctc_graph_beam_logp");
    return 0;
}

extern "C" int oe_ctc_graph_beam_logp_grad(const oe_ctc_graph_beam_logp_grad_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph_beam_logp_grad: null args");
    const oe_ctc_graph_beam_logp_grad_args& a = *args;
    if (int rc = bl_check("oe_ctc_graph_beam_logp_grad", a.graph, a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.workspace, a.max_active, a.beam,
                          a.status, a.peak))
        return rc;
    OE_REQUIRE(a.g && a.dlogits, "oe_ctc_graph_beam_logp_grad: null pointer (g / dlogits)");
    OE_REQUIRE(a.dlogits != a.logits, "oe_ctc_graph_beam_logp_grad: dlogits may not alias logits");
    OE_REQUIRE(a.normalized == 0, "oe_ctc_graph_beam_logp_grad: the gradient is with respect to raw logits (normalized must be 0)");
    const oe_beam_logp_graph& g = *a.graph;
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)a.B * a.T;                                       // oe_lp_rows holds them to the grid limit
    char* ws = reinterpret_cast<char*>(a.workspace);
    float* cw = reinterpret_cast<float*>(ws);
    ws += bl_rows_bytes(a.B, a.T, g.U);
    beam_u64* occ = reinterpret_cast<beam_u64*>(ws);
    ws += 2 * bl_rows_bytes(a.B, a.T, g.U);
    float* lse = reinterpret_cast<float*>(ws);
    ws += bl_up16((size_t)rows * 4);
    double* logz = reinterpret_cast<double*>(ws);
    ws += bl_up16((size_t)a.B * 8);
    if (int rc = oe_lp_rows("oe_ctc_graph_beam_logp_grad", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, g.cols, g.U, 0, cw, lse, st)) return rc;
    BlParams p = bl_params(true, g, cw, ws, a.T, a.hlens, a.max_active, a.beam);
    p.logp = a.logp; p.status = a.status; p.peak = a.peak; p.logz = logz; p.occ = occ;
    hipLaunchKernelGGL(bl_kernel<true>, dim3((unsigned)a.B), dim3(BL_BLOCK), 0, st, p);
    OE_LAUNCH_CHECK("ctc_graph_beam_logp_grad");
    hipLaunchKernelGGL(bl_dense_kernel, dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, a.logits, a.ldv, rows, a.T, a.V, a.hlens, a.g, logz, lse,
                       occ, g.U, g.inv, g.n_inv, a.dlogits);
    OE_LAUNCH_CHECK("ctc_graph_beam_logp_dense");
    return 0;
}
