// Graph CTC likelihood and its gradient: oe_ctc_graph's recursion in the log semiring.  The semantics every layer refers to
// are in include/openeat_hip.h (oe_ctc_graph_logp).
//
//   launch 1  lp_rows_kernel (lp_rows.hip): lp as a compact row of U + 1 floats; for the gradient it also keeps the row's log-sum-exp.
//   launch 2  gl_kernel: ONE WORKGROUP of 1024 threads PER UTTERANCE, the state in LDS as float64 in the log2 domain with a
//             finite "log 0" (ctc_f64.h's scheme: exp / log in float32 on differences).  A frame is two phases with a barrier
//             behind each:
//             A  per node q, over its groups (the arcs into q of one label, host-ordered): G[g] = LSE of the group's r; a
//                forward sweep leaves LSE(n_{t-1}[q], the groups before g) in X[g], a backward sweep combines the groups behind
//                g into it, so X[g] = "the node and every incoming arc of another label" without a subtraction; tot[q] = the
//                node and all groups.  n itself is not stored: n_t[q] = lp[t,0] + tot_t[q].  A node of more than 32 incoming
//                arcs takes a wave: a lane per run of groups and a log-semiring scan across the lanes, in both directions.
//             B  per arc a: r_t[a] = lp[t,label] + LSE(r_{t-1}[a], w[a] + (xg[a] >= 0 ? X[xg[a]] : tot[src[a]])).
//             LDS: 24 bytes per arc (r, X, G) and 8 per node (tot).
//             logZ: a fixed-order workgroup LSE over the final states.  The score ends here.
//             The gradient keeps alpha per frame in its workspace, then runs the mirror image over the out-groups (beta), and
//             per frame sums exp2(alpha + beta - logZ) per column over the column's arcs in the host's by-column order (a
//             thread per column; a wave for a column of more than 32 arcs) and over the nodes for the blank (one wave).
//             The thread's first arc keeps its constants in registers and has its lp of the next frame in flight (GL_PF).
//   launch 3  gl_dense_kernel (gradient): a wave per dlogits row: g * (occ scattered to its columns - softmax), zeros for
//             t >= Tb and for an infeasible utterance.
// Every sum runs in an order the code fixes.  No workgroup waits for another, no float atomics, no allocation, no host read.
#include <stdlib.h>
#include "oe_common.h"
#include "ctc_f64.h"
#include "../../include/openeat_hip.h"

#define GL_BLOCK 1024
#define GL_WAVES (GL_BLOCK / 64)
#define GL_PF 1                                   // frames of lp in flight ahead of the recursion (a thread's first arc)
#define GL_MAX_T (1 << 20)
#define GL_MAX_A OE_CTC_GRAPH_LOGP_MAX_ARCS
#define GL_MAX_Q OE_CTC_GRAPH_LOGP_MAX_NODES
#define GL_HEAVY 32                               // more arcs than this: a wave, not a thread
#define GL_MAX_HEAVY (GL_MAX_A / (GL_HEAVY + 1) + 1)
#define GL_NEG (-1.0e30)
#define GL_LOG2E 1.4426950408889634
#define GL_LN2 0.6931471805599453

static_assert(24 * GL_MAX_A + 8 * GL_MAX_Q + 3 * 2 * GL_MAX_HEAVY + 1024 <= 160 * 1024, "oe_ctc_graph_logp: the limits exceed the LDS");
static_assert(GL_MAX_Q >= 2048 && GL_MAX_A >= 4096, "oe_ctc_graph_logp: the limits are below what its users were promised");
static_assert(GL_MAX_Q <= 0xffff && GL_MAX_A <= 0xffff, "oe_ctc_graph_logp: the heavy lists hold 16-bit indices");

// ---------------------------------------------------------------- launch 2 ----
struct GlParams {
    const float* cw; int T, U, G, Qmax, Amax;
    const int* hlens; const int* graph_of; const int* node_off; const int* arc_off;
    const int* src; const int* dst; const int* col; const float* w; const float* fin;
    const int* in_gptr; const int* in_gstart; const int* in_perm; const int* in_xg;
    const int* out_gptr; const int* out_gstart; const int* out_perm; const int* out_xg;
    const int* col_ptr; const int* col_perm;
    float* logp; double* logz; double* alpha; float* occ;
};

// log2(2^a + 2^b): commutative bit for bit, and exact (= the other) against "log 0"
__device__ __forceinline__ double gl_lse(double a, double b) {
    const double m = fmax(a, b);
    return m + (double)nb_log2(1.f + nb_exp2((float)(fmin(a, b) - m)));
}
// a product into the log2 domain, pinned so that no instantiation fuses it into a neighbouring sum: the score's and the
// gradient's forward recursions must agree in every bit
__device__ __forceinline__ double gl_scale(float x) {
    double v = (double)x * GL_LOG2E;
    asm volatile("" : "+v"(v));
    return v;
}
// lp in the log2 domain; -inf (a masked log-probability) and NaN become "log 0"
__device__ __forceinline__ double gl_lp(float x) { return gl_scale(fmaxf(x, -1.0e30f)); }
__device__ __forceinline__ int gl_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }

__device__ __forceinline__ double gl_shfl_up(double v, int o) {
    const int lo = __shfl_up(__double2loint(v), o, 64), hi = __shfl_up(__double2hiint(v), o, 64);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double gl_shfl_down(double v, int o) {
    const int lo = __shfl_down(__double2loint(v), o, 64), hi = __shfl_down(__double2hiint(v), o, 64);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double gl_shfl(double v, int l) {
    const int lo = __shfl(__double2loint(v), l, 64), hi = __shfl(__double2hiint(v), l, 64);
    return __hiloint2double(hi, lo);
}

// The groups' tables of one direction, held to their ranges.
struct GlGroups {
    const int* gptr; const int* gstart; const int* perm; int A;
    __device__ __forceinline__ int lo(int q) const { return gl_clamp(gptr[q], 0, A); }
    __device__ __forceinline__ int start(int g) const { return gl_clamp(gstart[g], 0, A); }
    __device__ __forceinline__ int arc(int i) const { return gl_clamp(perm[i], 0, A - 1); }
};

// LSE of the group's values
template <class Val>
__device__ __forceinline__ double gl_group(const GlGroups& t, int g, Val val) {
    const int lo = t.start(g), hi = max(t.start(g + 1), lo);
    if (lo >= hi) return GL_NEG;
    double s = val(t.arc(lo));
    for (int i = lo + 1; i < hi; ++i) s = gl_lse(s, val(t.arc(i)));
    return s;
}

// A node by one thread: X[g] = LSE(stay, every group but g), returns LSE(stay, every group)
template <class Val>
__device__ __forceinline__ double gl_node_thread(const GlGroups& t, int gl, int gh, double stay, double* X, double* Gv, Val val) {
    double run = stay;
    for (int g = gl; g < gh; ++g) {
        const double s = gl_group(t, g, val);
        Gv[g] = s;
        X[g] = run;
        run = gl_lse(run, s);
    }
    if (gh - gl >= 2) {
        double suf = Gv[gh - 1];
        for (int g = gh - 2; g >= gl; --g) {
            X[g] = gl_lse(X[g], suf);
            suf = gl_lse(suf, Gv[g]);
        }
    }
    return run;
}

// A node by one wave: lane l takes the groups gl + l*per .. ; the lanes' totals are scanned in both directions
template <class Val>
__device__ __forceinline__ double gl_node_wave(const GlGroups& t, int lane, int gl, int gh, double stay, double* X, double* Gv, Val val) {
    const int per = (gh - gl + 63) / 64;
    const int lo = min(gl + lane * per, gh), hi = min(lo + per, gh);
    double run = GL_NEG;
    for (int g = lo; g < hi; ++g) {
        const double s = gl_group(t, g, val);
        Gv[g] = s;
        X[g] = run;
        run = gl_lse(run, s);
    }
    double pre = run, suf = run;                                             // inclusive scans of the lanes' totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = gl_shfl_up(pre, o), z = gl_shfl_down(suf, o);
        if (lane >= o) pre = gl_lse(pre, y);
        if (lane + o < 64) suf = gl_lse(suf, z);
    }
    const double total = gl_lse(stay, gl_shfl(pre, 63));
    double before = gl_shfl_up(pre, 1), behind = gl_shfl_down(suf, 1);
    before = lane == 0 ? stay : gl_lse(stay, before);
    if (lane == 63) behind = GL_NEG;
    for (int g = hi - 1; g >= lo; --g) {
        X[g] = gl_lse(gl_lse(before, X[g]), behind);
        behind = gl_lse(behind, Gv[g]);
    }
    return total;
}

template <bool GRAD>
__global__ __launch_bounds__(GL_BLOCK) void gl_kernel(const GlParams p) {
    extern __shared__ __attribute__((aligned(16))) double gl_sh[];
    __shared__ unsigned short heavy_in[GL_MAX_HEAVY], heavy_out[GL_MAX_HEAVY], heavy_col[GL_MAX_HEAVY];
    __shared__ int n_heavy[3];
    __shared__ double red[GL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int T = p.T, U = p.U;
    const int gi = p.graph_of ? gl_clamp(p.graph_of[b], 0, p.G - 1) : 0;
    const int q0 = p.node_off[gi], a0 = p.arc_off[gi];
    const int Q = gl_clamp(p.node_off[gi + 1] - q0, 1, p.Qmax), A = gl_clamp(p.arc_off[gi + 1] - a0, 0, p.Amax);
    double* r = gl_sh;
    double* X = r + p.Amax;
    double* Gv = X + p.Amax;
    double* tot = Gv + p.Amax;
    const int* src = p.src + a0; const int* dst = p.dst + a0; const int* col = p.col + a0;
    const float* w = p.w + a0; const float* fin = p.fin + q0;
    const GlGroups tin = {p.in_gptr + q0 + gi, p.in_gstart + a0 + gi, p.in_perm + a0, A};
    const GlGroups tout = {p.out_gptr + q0 + gi, p.out_gstart + a0 + gi, p.out_perm + a0, A};
    const int* in_xg = p.in_xg + a0; const int* out_xg = p.out_xg + a0;
    const int* col_ptr = p.col_ptr + (long)gi * (U + 1); const int* col_perm = p.col_perm + a0;
    const int Tb = max(min(p.hlens[b], T), 0);
    const long rw = U + 1;
    const float* cw = p.cw + (long)b * T * rw;
    const long astride = (long)p.Qmax + p.Amax;
    double* alpha = GRAD ? p.alpha + (long)b * T * astride : nullptr;

    // ---- before frame 0: n[0] = 0 (kept as tot with a zero lp), everything else unreachable; the lists of wide nodes / columns
    for (int a = tid; a < A; a += GL_BLOCK) r[a] = GL_NEG;
    for (int q = tid; q < Q; q += GL_BLOCK) tot[q] = q == 0 ? 0.0 : GL_NEG;
    if (tid < 3) n_heavy[tid] = 0;
    __syncthreads();
    auto arcs_of = [&](const GlGroups& t, int q) { const int gl = t.lo(q), gh = max(t.lo(q + 1), gl); return gl < gh ? max(t.start(gh) - t.start(gl), 0) : 0; };
    for (int q = tid; q < Q; q += GL_BLOCK) {                                // the order of a list does not reach the results
        if (arcs_of(tin, q) > GL_HEAVY) { const int i = atomicAdd(&n_heavy[0], 1); if (i < GL_MAX_HEAVY) heavy_in[i] = (unsigned short)q; }
        if (GRAD && arcs_of(tout, q) > GL_HEAVY) { const int i = atomicAdd(&n_heavy[1], 1); if (i < GL_MAX_HEAVY) heavy_out[i] = (unsigned short)q; }
    }
    auto col_lo = [&](int k) { return gl_clamp(col_ptr[k], 0, A); };
    if (GRAD)
        for (int k = tid; k < U; k += GL_BLOCK)
            if (col_lo(k + 1) - col_lo(k) > GL_HEAVY) { const int i = atomicAdd(&n_heavy[2], 1); if (i < GL_MAX_HEAVY) heavy_col[i] = (unsigned short)k; }
    __syncthreads();
    const int nh_in = min(n_heavy[0], GL_MAX_HEAVY), nh_out = min(n_heavy[1], GL_MAX_HEAVY), nh_col = min(n_heavy[2], GL_MAX_HEAVY);

    // the thread's first arc: its constants in registers, its lp a frame ahead
    const bool has0 = tid < A;
    int s0 = 0, d0 = 0, k0 = 0, xi0 = -1, xo0 = -1;
    double w0 = 0.0;
    float lp_next = 0.f;
    if (has0) {
        s0 = gl_clamp(src[tid], 0, Q - 1);
        d0 = gl_clamp(dst[tid], 0, Q - 1);
        k0 = gl_clamp(col[tid], 0, U - 1);
        xi0 = gl_clamp(in_xg[tid], -1, A - 1);
        xo0 = GRAD ? gl_clamp(out_xg[tid], -1, A - 1) : -1;
        w0 = gl_scale(w[tid]);
        if (Tb > 0) lp_next = cw[1 + k0];
    }

    // ---- alpha
    double lp0_prev = 0.0;
    for (int t = 0; t < Tb; ++t) {
        const float* row = cw + (long)t * rw;
        const double lp0 = gl_lp(row[0]);
        const float lp_a0 = lp_next;
        if (has0 && t + GL_PF < Tb) lp_next = row[rw + 1 + k0];
        double* al = GRAD ? alpha + (long)t * astride : nullptr;
        auto val = [&](int a) { return r[a]; };
        // phase A: per node, the exclusions of frame t-1 and n_t
        for (int q = tid; q < Q; q += GL_BLOCK) {
            const int gl = tin.lo(q), gh = max(tin.lo(q + 1), gl);
            if (arcs_of(tin, q) > GL_HEAVY) continue;
            const double v = gl_node_thread(tin, gl, gh, lp0_prev + tot[q], X, Gv, val);
            tot[q] = v;
            if (GRAD) al[q] = lp0 + v;
        }
        for (int i = wave; i < nh_in; i += GL_WAVES) {
            const int q = heavy_in[i];
            const int gl = tin.lo(q), gh = max(tin.lo(q + 1), gl);
            const double v = gl_node_wave(tin, lane, gl, gh, lp0_prev + tot[q], X, Gv, val);
            if (lane == 0) {
                tot[q] = v;
                if (GRAD) al[q] = lp0 + v;
            }
        }
        __syncthreads();
        // phase B: per arc
        for (int a = tid; a < A; a += GL_BLOCK) {
            int s, x;
            double wa, lp;
            if (a == tid) { s = s0; x = xi0; wa = w0; lp = gl_lp(lp_a0); }
            else {
                s = gl_clamp(src[a], 0, Q - 1);
                x = gl_clamp(in_xg[a], -1, A - 1);
                wa = gl_scale(w[a]);
                lp = gl_lp(row[1 + gl_clamp(col[a], 0, U - 1)]);
            }
            const double v = lp + gl_lse(r[a], wa + (x >= 0 ? X[x] : tot[s]));
            r[a] = v;
            if (GRAD) al[p.Qmax + a] = v;
        }
        __syncthreads();
        lp0_prev = lp0;
    }

    // ---- logZ: nodes then arcs per thread, the lanes by a butterfly (gl_lse is commutative), the waves in order
    auto fin2 = [&](int q) { return fmax(gl_scale(fin[q]), GL_NEG); };
    double z = GL_NEG;
    if (Tb > 0) {
        for (int q = tid; q < Q; q += GL_BLOCK) z = gl_lse(z, (lp0_prev + tot[q]) + fin2(q));
        for (int a = tid; a < A; a += GL_BLOCK) z = gl_lse(z, r[a] + fin2(gl_clamp(dst[a], 0, Q - 1)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z = gl_lse(z, oe_shfl_xor_f64(z, o));
    if (lane == 0) red[wave] = z;
    __syncthreads();
    z = red[0];
    for (int i = 1; i < GL_WAVES; ++i) z = gl_lse(z, red[i]);
    const bool ok = Tb > 0 && z > 0.5 * GL_NEG;
    if (tid == 0) {
        if (p.logp) p.logp[b] = ok ? (float)(z * GL_LN2) : -INFINITY;
        if (GRAD) p.logz[b] = ok ? z : GL_NEG;
    }
    if (!GRAD || !ok) return;

    // ---- beta and the occupancies.  r = beta of the arc states, tot = beta of the node states.
    float* occ = p.occ + (long)b * T * rw;
    auto blank_occ = [&](int t) {                                             // one wave: the nodes by lane, then a butterfly
        if (wave != GL_WAVES - 1) return;
        const double* al = alpha + (long)t * astride;
        float s = 0.f;
        for (int q = lane; q < Q; q += 64) s += nb_exp2((float)(al[q] + tot[q] - z));
        s = wave_sum(s);
        if (lane == 0) occ[(long)t * rw] = s;
    };
    auto arc_occ = [&](int t) {
        const double* al = alpha + (long)t * astride + p.Qmax;
        float* oc = occ + (long)t * rw + 1;
        for (int k = tid; k < U; k += GL_BLOCK) {
            const int lo = col_lo(k), hi = col_lo(k + 1);
            if (hi - lo > GL_HEAVY) continue;
            float s = 0.f;
            for (int i = lo; i < hi; ++i) {
                const int a = gl_clamp(col_perm[i], 0, A - 1);
                s += nb_exp2((float)(al[a] + r[a] - z));
            }
            oc[k] = s;
        }
        for (int j = wave; j < nh_col; j += GL_WAVES) {
            const int k = heavy_col[j];
            const int lo = col_lo(k), hi = col_lo(k + 1);
            float s = 0.f;
            for (int i = lo + lane; i < hi; i += 64) {
                const int a = gl_clamp(col_perm[i], 0, A - 1);
                s += nb_exp2((float)(al[a] + r[a] - z));
            }
            s = wave_sum(s);
            if (lane == 0) oc[k] = s;
        }
    };
    __syncthreads();                                                         // every wave has read tot and r for logZ
    for (int a = tid; a < A; a += GL_BLOCK) r[a] = fin2(gl_clamp(dst[a], 0, Q - 1));
    for (int q = tid; q < Q; q += GL_BLOCK) tot[q] = fin2(q);
    if (has0 && Tb > 1) lp_next = cw[(long)(Tb - 1) * rw + 1 + k0];
    __syncthreads();
    blank_occ(Tb - 1);
    __syncthreads();
    for (int t = Tb - 2; t >= 0; --t) {
        const float* row = cw + (long)(t + 1) * rw;                           // beta_t reads lp of frame t + 1
        const double lp0 = gl_lp(row[0]);
        const float lp_a0 = lp_next;
        if (has0 && t - GL_PF >= 0) lp_next = row[1 + k0 - rw];
        auto val = [&](int a) { return (gl_scale(w[a]) + gl_lp(row[1 + gl_clamp(col[a], 0, U - 1)])) + r[a]; };
        // phase A: per node over its out-groups; the arcs' occupancies of frame t + 1 (they read r, as this phase does)
        for (int q = tid; q < Q; q += GL_BLOCK) {
            const int gl = tout.lo(q), gh = max(tout.lo(q + 1), gl);
            if (arcs_of(tout, q) > GL_HEAVY) continue;
            tot[q] = gl_node_thread(tout, gl, gh, lp0 + tot[q], X, Gv, val);
        }
        for (int i = wave; i < nh_out; i += GL_WAVES) {
            const int q = heavy_out[i];
            const int gl = tout.lo(q), gh = max(tout.lo(q + 1), gl);
            const double v = gl_node_wave(tout, lane, gl, gh, lp0 + tot[q], X, Gv, val);
            if (lane == 0) tot[q] = v;
        }
        arc_occ(t + 1);
        __syncthreads();
        // phase B: per arc; the nodes' occupancy of frame t (it reads tot, as this phase does)
        for (int a = tid; a < A; a += GL_BLOCK) {
            int d, x;
            double lp;
            if (a == tid) { d = d0; x = xo0; lp = gl_lp(lp_a0); }
            else {
                d = gl_clamp(dst[a], 0, Q - 1);
                x = gl_clamp(out_xg[a], -1, A - 1);
                lp = gl_lp(row[1 + gl_clamp(col[a], 0, U - 1)]);
            }
            r[a] = gl_lse(lp + r[a], x >= 0 ? X[x] : tot[d]);
        }
        blank_occ(t);
        __syncthreads();
    }
    arc_occ(0);
}

// ---------------------------------------------------------------- launch 3 ----
// One wave per dlogits row.
__global__ __launch_bounds__(256) void gl_dense_kernel(const float* __restrict__ logits, long ldv, long rows, int T, int V,
                                                        const int* __restrict__ hlens, const float* __restrict__ g,
                                                        const double* __restrict__ logz, const float* __restrict__ lse,
                                                        const float* __restrict__ occ, int U, const int* __restrict__ inv, int n_inv,
                                                        float* __restrict__ dlogits) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (int)(row / T), t = (int)(row % T);
    float* dl = dlogits + row * ldv;
    if (t >= hlens[b] || !(logz[b] > 0.5 * GL_NEG)) {                         // g of an infeasible utterance is not read
        for (int v = lane; v < V; v += 64) dl[v] = 0.f;
        return;
    }
    const float gb = g[b], c = lse[row];
    const float* x = logits + row * ldv;
    const float* oc = occ + row * (long)(U + 1);
    for (int v = lane; v < V; v += 64) {
        const int k = v < n_inv ? min(inv[v], U) : -1;
        const float o = k >= 0 ? oc[k] : 0.f;
        dl[v] = gb * (o - expf(x[v] - c));
    }
}

// ---------------------------------------------------------------- host -------
static bool gl_shape_ok(long B, long T, long U, long Q, long A) {
    return B > 0 && T > 0 && T <= GL_MAX_T && U > 0 && Q >= 1 && Q <= GL_MAX_Q && A >= 1 && A <= GL_MAX_A;
}
static size_t gl_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static size_t gl_rows_bytes(int B, int T, int U) { return gl_up16((size_t)B * (size_t)T * ((size_t)U + 1) * 4); }

extern "C" size_t oe_ctc_graph_logp_workspace_bytes(int B, int T, int U, int Qmax, int Amax) {
    if (!gl_shape_ok(B, T, U, Qmax, Amax)) return 0;
    return (size_t)B * (size_t)T * ((size_t)U + 1) * 4;
}

extern "C" size_t oe_ctc_graph_logp_grad_workspace_bytes(int B, int T, int U, int Qmax, int Amax) {
    if (!gl_shape_ok(B, T, U, Qmax, Amax)) return 0;
    return 2 * gl_rows_bytes(B, T, U) + gl_up16((size_t)B * (size_t)T * 4) + gl_up16((size_t)B * 8) +
           gl_up16((size_t)B * (size_t)T * ((size_t)Qmax + (size_t)Amax) * 8);
}

// the checks the two entries share; everything is reported before any launch
static int gl_check(const char* name, const float* logits, long ldv, int B, int T, int V, const int* hlens, const oe_graph_set* set,
                    void* workspace) {
    OE_REQUIRE(set, "%s: null set", name);
    const oe_graph_set& s = *set;
    OE_REQUIRE(logits, "%s: null logits", name);
    OE_REQUIRE(hlens, "%s: null hlens", name);
    OE_REQUIRE(workspace, "%s: null workspace", name);
    OE_REQUIRE(B > 0 && T > 0 && T <= GL_MAX_T && V > 1 && ldv >= V, "%s: bad shape B=%d T=%d V=%d ldv=%ld (1 <= B, 1 <= T <= 2^20, ldv >= V)",
               name, B, T, V, ldv);
    OE_REQUIRE(s.G >= 1, "%s: G=%d graphs < 1", name, s.G);
    OE_REQUIRE(s.Qmax >= 1 && s.Qmax <= GL_MAX_Q, "%s: Qmax=%d nodes outside 1 .. %d (the node values live in LDS)", name, s.Qmax, GL_MAX_Q);
    OE_REQUIRE(s.Amax >= 1 && s.Amax <= GL_MAX_A, "%s: Amax=%d arcs outside 1 .. %d (the arc values live in LDS)", name, s.Amax, GL_MAX_A);
    OE_REQUIRE(s.U >= 1 && s.U < V, "%s: U=%d distinct labels outside 1 .. V-1 = %d", name, s.U, V - 1);
    OE_REQUIRE(s.n_inv >= 0, "%s: n_inv=%d < 0", name, s.n_inv);
    OE_REQUIRE(s.node_off && s.arc_off && s.in_ptr && s.src && s.dst && s.label && s.col && s.w && s.final && s.cols && s.in_gptr &&
                   s.in_gstart && s.in_perm && s.in_xg && s.out_gptr && s.out_gstart && s.out_perm && s.out_xg && s.col_ptr && s.col_perm &&
                   (s.inv || s.n_inv == 0),
               "%s: null table in set", name);
    OE_REQUIRE((((uintptr_t)workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", name);
    return 0;
}

static int gl_raise_lds(const char* name) {
    static bool raised = false;                                       // once per process: opt in to more than 64 KB of dynamic LDS
    if (!raised) {
        const int lds_max = 24 * GL_MAX_A + 8 * GL_MAX_Q;
        if (hipFuncSetAttribute((const void*)gl_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess ||
            hipFuncSetAttribute((const void*)gl_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess) {
            oe_set_error("%s: cannot raise the dynamic LDS limit", name);
            return -1;
        }
        raised = true;
    }
    return 0;
}

static GlParams gl_params(const oe_graph_set& s, const float* cw, int T, const int* hlens, const int* graph_of) {
    GlParams p;
    p.cw = cw; p.T = T; p.U = s.U; p.G = s.G; p.Qmax = s.Qmax; p.Amax = s.Amax;
    p.hlens = hlens; p.graph_of = graph_of; p.node_off = s.node_off; p.arc_off = s.arc_off;
    p.src = s.src; p.dst = s.dst; p.col = s.col; p.w = s.w; p.fin = s.final;
    p.in_gptr = s.in_gptr; p.in_gstart = s.in_gstart; p.in_perm = s.in_perm; p.in_xg = s.in_xg;
    p.out_gptr = s.out_gptr; p.out_gstart = s.out_gstart; p.out_perm = s.out_perm; p.out_xg = s.out_xg;
    p.col_ptr = s.col_ptr; p.col_perm = s.col_perm;
    p.logp = nullptr; p.logz = nullptr; p.alpha = nullptr; p.occ = nullptr;
    return p;
}

extern "C" int oe_ctc_graph_logp(const oe_ctc_graph_logp_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph_logp: null args");
    const oe_ctc_graph_logp_args& a = *args;
    if (int rc = gl_check("oe_ctc_graph_logp", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.set, a.workspace)) return rc;
    OE_REQUIRE(a.logp, "oe_ctc_graph_logp: null logp");
    const oe_graph_set& s = *a.set;
    const size_t lds = 24 * (size_t)s.Amax + 8 * (size_t)s.Qmax;
    if (lds > 48 * 1024)
        if (int rc = gl_raise_lds("oe_ctc_graph_logp")) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* cw = reinterpret_cast<float*>(a.workspace);
    if (int rc = oe_lp_rows("oe_ctc_graph_logp", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, s.cols, s.U, a.normalized, cw, nullptr, st))
        return rc;
    GlParams p = gl_params(s, cw, a.T, a.hlens, a.graph_of);
    p.logp = a.logp;
    hipLaunchKernelGGL(gl_kernel<false>, dim3((unsigned)a.B), dim3(GL_BLOCK), lds, st, p);
    OE_LAUNCH_CHECK("ctc_graph_logp");
    return 0;
}

extern "C" int oe_ctc_graph_logp_grad(const oe_ctc_graph_logp_grad_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph_logp_grad: null args");
    const oe_ctc_graph_logp_grad_args& a = *args;
    if (int rc = gl_check("oe_ctc_graph_logp_grad", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.set, a.workspace)) return rc;
    OE_REQUIRE(a.g && a.dlogits, "oe_ctc_graph_logp_grad: null pointer (g / dlogits)");
    OE_REQUIRE(a.dlogits != a.logits, "oe_ctc_graph_logp_grad: dlogits may not alias logits");
    OE_REQUIRE(a.normalized == 0, "oe_ctc_graph_logp_grad: the gradient is with respect to raw logits (normalized must be 0)");
    const oe_graph_set& s = *a.set;
    const size_t lds = 24 * (size_t)s.Amax + 8 * (size_t)s.Qmax;
    if (lds > 48 * 1024)
        if (int rc = gl_raise_lds("oe_ctc_graph_logp_grad")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)a.B * a.T;                                       // oe_lp_rows holds them to the grid limit
    char* ws = reinterpret_cast<char*>(a.workspace);
    float* cw = reinterpret_cast<float*>(ws);
    ws += gl_rows_bytes(a.B, a.T, s.U);
    float* occ = reinterpret_cast<float*>(ws);
    ws += gl_rows_bytes(a.B, a.T, s.U);
    float* lse = reinterpret_cast<float*>(ws);
    ws += gl_up16((size_t)rows * 4);
    double* logz = reinterpret_cast<double*>(ws);
    ws += gl_up16((size_t)a.B * 8);
    double* alpha = reinterpret_cast<double*>(ws);
    if (int rc = oe_lp_rows("oe_ctc_graph_logp_grad", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, s.cols, s.U, 0, cw, lse, st)) return rc;
    GlParams p = gl_params(s, cw, a.T, a.hlens, a.graph_of);
    p.logp = a.logp; p.logz = logz; p.alpha = alpha; p.occ = occ;
    hipLaunchKernelGGL(gl_kernel<true>, dim3((unsigned)a.B), dim3(GL_BLOCK), lds, st, p);
    OE_LAUNCH_CHECK("ctc_graph_logp_grad");
    hipLaunchKernelGGL(gl_dense_kernel, dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, a.logits, a.ldv, rows, a.T, a.V, a.hlens, a.g, logz, lse,
                       occ, s.U, s.inv, s.n_inv, a.dlogits);
    OE_LAUNCH_CHECK("ctc_graph_logp_dense");
    return 0;
}
