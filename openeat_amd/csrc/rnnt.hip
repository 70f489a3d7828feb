// Transducer (RNN-T) loss and gradient, and the joint network's broadcast.  The semantics every layer refers to are in
// include/openeat_hip.h (oe_rnnt_loss, oe_rnnt_grad, oe_joint_combine_fwd / _bwd).
//
//   launch 1  rt_rows_kernel: ONE WAVE PER LATTICE NODE (b,t,u) with t < Tb, u <= Ub.  One pass over the node's V logits
//             (16-byte loads behind an unaligned head, a running max and sum per lane, merged across the wave): the row's
//             log-sum-exp [b][t][u] for the gradient pass, and lp of the blank and of the next label as (x - max) - log(sum),
//             laid out [b][u][t] so that a lane of the recursion walks t contiguously.  Nodes outside the lattice are not read.
//   launch 2  rt_lattice_kernel: ONE WORKGROUP OF TWO WAVES PER UTTERANCE, wave 0 alpha and wave 1 beta.  Lane l holds the NS
//             label positions l*NS .. l*NS+NS-1 (NS = 1, 2, 4 for U1 <= 64, 128, 256); a step is an anti-diagonal d = t + u.
//             alpha: a position's blank predecessor is its own previous value, its label predecessor the lower neighbour's
//             previous value - inside the lane, or by one DPP shift from the lane below (nb_shr1); beta the mirror image with
//             nb_shl1.  State float64 in the log2 domain with the finite "log 0" of ctc_f64.h, exp / log float32 on
//             differences; lp is fetched RT_CH(NS) = 16, 8, 4 steps ahead.  Writes alpha, beta [b][u][t], logZ (log2 domain) and logp.
//             The wave of alpha also checks what only the device can see (ulens, the targets): status, logp = -inf.
//   launch 3  rt_grad_kernel: ONE WAVE PER NODE of the (B, T, U1) grid: reads the row again and writes
//             g * ([v = blank] e_b + [v = y] e_y - (e_b + e_y) * softmax) - zeros outside the lattice and for an infeasible
//             utterance.  Each element is read and then written by the same lane: dlogits may be the logits buffer.
// No float atomics, every sum in a fixed order, no workgroup waits for another, no allocation, no host read.
#include "oe_common.h"
#include "ctc_f64.h"
#include "../../include/openeat_hip.h"

#define RT_CH(NS) (16 / (NS))                     // steps of lp in flight ahead of the recursion: 32 floats a lane, twice
#define RT_ROW_UNROLL 4                           // 16-byte loads a lane of the row and gradient passes issues before it uses one
#define RT_LOG2E 1.4426950408889634
#define RT_LN2 0.6931471805599453

// lp in the log2 domain; -inf and NaN become "log 0"
__device__ __forceinline__ double rt_lp2(float x) { return (double)fmaxf(x, -1.0e30f) * RT_LOG2E; }
__device__ __forceinline__ int rt_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }

struct RtWs {
    float* lse; float* lpb; float* lpl; double* alpha; double* beta; double* logz; int* status;
};

// ---------------------------------------------------------------- launch 1 ----
// A wave over the V values of one row: f(v, x) for every v < V once, 16-byte loads where the address allows.
template <class F>
__device__ __forceinline__ void rt_row_read(const float* __restrict__ x, int V, int lane, F f) {
    const int head = min((int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2), V);
    if (lane < head) f(lane, x[lane]);
    const int n4 = (V - head) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + head);
    for (int i0 = lane; i0 < n4; i0 += 64 * RT_ROW_UNROLL) {                  // RT_ROW_UNROLL loads in flight before the first use
        float4 q[RT_ROW_UNROLL];
#pragma unroll
        for (int k = 0; k < RT_ROW_UNROLL; ++k)
            if (i0 + 64 * k < n4) q[k] = x4[i0 + 64 * k];
#pragma unroll
        for (int k = 0; k < RT_ROW_UNROLL; ++k)
            if (i0 + 64 * k < n4) {
                const int v = head + 4 * (i0 + 64 * k);
                f(v, q[k].x); f(v + 1, q[k].y); f(v + 2, q[k].z); f(v + 3, q[k].w);
            }
    }
    const int tail = head + 4 * n4;
    if (tail + lane < V) f(tail + lane, x[tail + lane]);
}

__global__ __launch_bounds__(256) void rt_rows_kernel(const float* __restrict__ logits, long ldv, long nodes, int T, int U1, int V,
                                                       const int* __restrict__ hlens, const int* __restrict__ targets,
                                                       const int* __restrict__ ulens, int blank, RtWs w) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= nodes) return;
    const int b = (int)(n / ((long)T * U1));
    const int r = (int)(n - (long)b * T * U1);
    const int t = r / U1, u = r - t * U1;
    const int Tb = rt_clamp(hlens[b], 0, T), Ub = rt_clamp(ulens[b], 0, U1 - 1);
    if (t >= Tb || u > Ub) return;
    const float* x = logits + n * ldv;
    float m = -INFINITY, s = 0.f;
    rt_row_read(x, V, lane, [&](int, float v) {
        const float mn = fmaxf(m, v);
        s = s * __expf(m - mn) + __expf(v - mn);          // m = -inf at first: s = 0 * 0 + 1
        m = mn;
    });
    wave_lse(m, s);
    if (lane == 0) {
        const float ls = __logf(s);
        const int y = u < Ub ? rt_clamp(targets[(long)b * (U1 - 1) + u], 0, V - 1) : blank;
        const long k = ((long)b * U1 + u) * T + t;
        w.lse[n] = m + ls;
        w.lpb[k] = (x[blank] - m) - ls;
        w.lpl[k] = u < Ub ? (x[y] - m) - ls : 0.f;
    }
}

// ---------------------------------------------------------------- launch 2 ----
// One direction over the Tb + Ub anti-diagonals of an utterance.  lpb, lpl, out: the utterance's [u][t] planes.  Step k reads
// lp at time  FWD ? k - u : Tb-1 + Ub - u - k  of position u: alpha takes lp of the node it leaves (its own previous t), beta
// of the node it makes.  Returns the state after the last step (alpha(Tb-1, u) / beta(0, u) where the lane holds it).
template <bool FWD, int NS, int CH>
__device__ __forceinline__ void rt_recurse(int lane, int T, int Tb, int Ub, const float* __restrict__ lpb, const float* __restrict__ lpl,
                                           double* __restrict__ out, double (&a)[NS]) {
    const int steps = FWD ? Tb - 1 + Ub : Tb + Ub;
    bool valid[NS];
    int t0[NS];                                     // the time step 0 reads
    const float* pb[NS]; const float* pl[NS]; double* po[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int u = lane * NS + j;
        valid[j] = u <= Ub;
        const long row = (long)min(u, Ub) * T;      // in bounds whether or not it is used
        pb[j] = lpb + row; pl[j] = lpl + row; po[j] = out + row;
        t0[j] = FWD ? -u : Tb - 1 + Ub - u;
        a[j] = (u == (FWD ? 0 : Ub)) ? 0.0 : NB_NEG_D;   // alpha(0,0) = 0; beta: the value "behind" (Tb-1, Ub) is 0
    }
    if (FWD && lane == 0) po[0][0] = 0.0;
    auto fetch = [&](int k, float (&fb)[NS], float (&fl)[NS]) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int t = FWD ? t0[j] + k : t0[j] - k;
            fb[j] = 0.f; fl[j] = 0.f;
            if (valid[j] && k < steps && t >= 0 && t < Tb) { fb[j] = pb[j][t]; fl[j] = pl[j][t]; }
        }
    };
    float cb[CH][NS], cl[CH][NS], nb[CH][NS], nl[CH][NS];
#pragma unroll
    for (int i = 0; i < CH; ++i) fetch(i, cb[i], cl[i]);
    for (int k0 = 0; k0 < steps; k0 += CH) {
#pragma unroll
        for (int i = 0; i < CH; ++i) fetch(k0 + CH + i, nb[i], nl[i]);
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int k = k0 + i;
            if (k < steps) {                           // wave-uniform
                double na[NS];
                if (FWD) {
                    double ey[NS];
#pragma unroll
                    for (int j = 0; j < NS; ++j) ey[j] = a[j] + rt_lp2(cl[i][j]);
                    const double below = nb_shr1(ey[NS - 1]);
#pragma unroll
                    for (int j = 0; j < NS; ++j) na[j] = nb_lse2_add(a[j] + rt_lp2(cb[i][j]), j >= 1 ? ey[j >= 1 ? j - 1 : 0] : below, 0.0);
                } else {
                    const double above = nb_shl1(a[0]);
#pragma unroll
                    for (int j = 0; j < NS; ++j)
                        na[j] = nb_lse2_add(a[j] + rt_lp2(cb[i][j]), (j + 1 < NS ? a[j + 1 < NS ? j + 1 : 0] : above) + rt_lp2(cl[i][j]), 0.0);
                }
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    const int t = FWD ? t0[j] + k + 1 : t0[j] - k;       // the time of the value just made
                    const bool in = valid[j] && t >= 0 && t < Tb;
                    a[j] = in ? na[j] : NB_NEG_D;
                    if (in) po[j][t] = a[j];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                cb[i][j] = nb[i][j]; cl[i][j] = nl[i][j];
                asm volatile("" : "+v"(cb[i][j]), "+v"(cl[i][j]));     // wait for the prefetch once per chunk
            }
    }
}

template <int NS>
__global__ __launch_bounds__(128) void rt_lattice_kernel(int T, int U1, int V, const int* __restrict__ hlens,
                                                          const int* __restrict__ targets, const int* __restrict__ ulens, int blank,
                                                          float* __restrict__ logp, int* __restrict__ status, RtWs w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int Tb = rt_clamp(hlens[b], 0, T);
    const int ul = ulens[b];
    const int Ub = rt_clamp(ul, 0, U1 - 1);
    // what only the device can see: the length and the labels (every lane of both waves reaches the same verdict)
    int bad = (ul < 0 || ul > U1 - 1) ? 1 : 0;
    for (int i = lane; i < Ub; i += 64) {
        const int y = targets[(long)b * (U1 - 1) + i];
        if (y < 0 || y >= V || y == blank) bad = 1;
    }
    bad = __any(bad) ? 1 : 0;
    const long plane = (long)b * U1 * T;
    if (bad || Tb <= 0) {
        if (wave == 0 && lane == 0) {
            logp[b] = -INFINITY;
            w.logz[b] = NB_NEG_D;
            w.status[b] = bad;
            if (status) status[b] = bad;
        }
        return;
    }
    double a[NS];
    if (wave == 0) {
        rt_recurse<true, NS, RT_CH(NS)>(lane, T, Tb, Ub, w.lpb + plane, w.lpl + plane, w.alpha + plane, a);
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (lane * NS + j == Ub) {
                const double z = a[j] + rt_lp2(w.lpb[plane + (long)Ub * T + Tb - 1]);
                const bool ok = z > 0.5 * NB_NEG_D;
                logp[b] = ok ? (float)(z * RT_LN2) : -INFINITY;
                w.logz[b] = ok ? z : NB_NEG_D;
                w.status[b] = 0;
                if (status) status[b] = 0;
            }
    } else {
        rt_recurse<false, NS, RT_CH(NS)>(lane, T, Tb, Ub, w.lpb + plane, w.lpl + plane, w.beta + plane, a);
    }
}

// ---------------------------------------------------------------- launch 3 ----
// A wave over the V values of one row, in place: x[v] <- f(v, x[v]), the read and the write of an element by the same lane.
template <class F>
__device__ __forceinline__ void rt_row_map(const float* x, float* y, int V, int lane, F f) {
    const int head = min((int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2), V);
    if (lane < head) y[lane] = f(lane, x[lane]);
    const int n4 = (V - head) >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + head);
    float4* y4 = reinterpret_cast<float4*>(y + head);
    for (int i0 = lane; i0 < n4; i0 += 64 * RT_ROW_UNROLL) {
        float4 q[RT_ROW_UNROLL];
#pragma unroll
        for (int k = 0; k < RT_ROW_UNROLL; ++k)
            if (i0 + 64 * k < n4) q[k] = x4[i0 + 64 * k];
#pragma unroll
        for (int k = 0; k < RT_ROW_UNROLL; ++k)
            if (i0 + 64 * k < n4) {
                const int v = head + 4 * (i0 + 64 * k);
                q[k].x = f(v, q[k].x); q[k].y = f(v + 1, q[k].y); q[k].z = f(v + 2, q[k].z); q[k].w = f(v + 3, q[k].w);
                y4[i0 + 64 * k] = q[k];
            }
    }
    const int tail = head + 4 * n4;
    if (tail + lane < V) y[tail + lane] = f(tail + lane, x[tail + lane]);
}

__global__ __launch_bounds__(256) void rt_grad_kernel(const float* logits, long ldv, long nodes, int T, int U1, int V,
                                                       const int* __restrict__ hlens, const int* __restrict__ targets,
                                                       const int* __restrict__ ulens, int blank, const float* __restrict__ g,
                                                       float* dlogits, RtWs w) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= nodes) return;
    const int b = (int)(n / ((long)T * U1));
    const int r = (int)(n - (long)b * T * U1);
    const int t = r / U1, u = r - t * U1;
    const int Tb = rt_clamp(hlens[b], 0, T), Ub = rt_clamp(ulens[b], 0, U1 - 1);
    const float* x = logits + n * ldv;
    float* dl = dlogits + n * ldv;
    const double z = w.logz[b];
    if (t >= Tb || u > Ub || !(z > 0.5 * NB_NEG_D)) {                        // g of an infeasible utterance is not read
        rt_row_map(x, dl, V, lane, [](int, float) { return 0.f; });          // same rows: dlogits has the layout of logits
        return;
    }
    const long plane = (long)b * U1 * T;
    const long k = plane + (long)u * T + t;
    const double al = w.alpha[k];
    float eb = 0.f, ey = 0.f;
    int y = -1;
    if (t + 1 < Tb) eb = nb_exp2((float)(al + rt_lp2(w.lpb[k]) + w.beta[k + 1] - z));
    else if (u == Ub) eb = nb_exp2((float)(al + rt_lp2(w.lpb[k]) - z));
    if (u < Ub) {
        y = rt_clamp(targets[(long)b * (U1 - 1) + u], 0, V - 1);
        ey = nb_exp2((float)(al + rt_lp2(w.lpl[k]) + w.beta[k + T] - z));
    }
    const float gb = g[b], c = w.lse[n];
    const float occ = eb + ey;
    rt_row_map(x, dl, V, lane, [&](int v, float xv) {
        float d = -occ * __expf(xv - c);
        if (v == blank) d += eb;
        if (v == y) d += ey;
        return gb * d;
    });
}

// ---------------------------------------------------------------- joint combine ----
__global__ __launch_bounds__(256) void jc_fwd_kernel(const float* __restrict__ e, const float* __restrict__ p, int T, int U1, int J, int act,
                                                      const int* __restrict__ hlens, const int* __restrict__ ulens, float* __restrict__ z) {
    const long bt = blockIdx.x;                                              // one workgroup per (b,t)
    const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
    const int Tb = hlens ? hlens[b] : T, Ub = ulens ? ulens[b] : U1 - 1;
    const float* er = e + bt * J;
    const float* pr = p + (long)b * U1 * J;
    float* zr = z + bt * U1 * J;
    for (int j = threadIdx.x; j < J; j += 256) {
        const float ev = er[j];
        for (int u = 0; u < U1; ++u) zr[(long)u * J + j] = (t < Tb && u <= Ub) ? act_fwd(act, ev + pr[(long)u * J + j]) : 0.f;
    }
}

// blocks [0, B*T): de of one (b,t), u ascending; blocks [B*T, B*T + B*U1): dp of one (b,u), t ascending
__global__ __launch_bounds__(256) void jc_bwd_kernel(const float* __restrict__ e, const float* __restrict__ p, int B, int T, int U1, int J,
                                                      int act, const int* __restrict__ hlens, const int* __restrict__ ulens,
                                                      const float* __restrict__ dz, float* __restrict__ de, float* __restrict__ dp) {
    const long blk = blockIdx.x, BT = (long)B * T;
    if (blk < BT) {
        const int b = (int)(blk / T), t = (int)(blk - (long)b * T);
        const int Tb = hlens ? hlens[b] : T, Ub = min(ulens ? ulens[b] : U1 - 1, U1 - 1);
        const float* pr = p + (long)b * U1 * J;
        const float* dr = dz + blk * U1 * J;
        for (int j = threadIdx.x; j < J; j += 256) {
            const float ev = e[blk * J + j];
            float s = 0.f;
            if (t < Tb)
                for (int u = 0; u <= Ub; ++u) s += dr[(long)u * J + j] * act_bwd(act, ev + pr[(long)u * J + j]);
            de[blk * J + j] = s;
        }
    } else {
        const long bu = blk - BT;
        const int b = (int)(bu / U1), u = (int)(bu - (long)b * U1);
        const int Tb = min(hlens ? hlens[b] : T, T), Ub = ulens ? ulens[b] : U1 - 1;
        const float* er = e + (long)b * T * J;
        const float* dr = dz + ((long)b * T * U1 + u) * J;
        for (int j = threadIdx.x; j < J; j += 256) {
            const float pv = p[bu * J + j];
            float s = 0.f;
            if (u <= Ub)
                for (int t = 0; t < Tb; ++t) s += dr[(long)t * U1 * J + j] * act_bwd(act, er[(long)t * J + j] + pv);
            dp[bu * J + j] = s;
        }
    }
}

// ---------------------------------------------------------------- host -------
static size_t rt_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static bool rt_shape_ok(long B, long T, long Umax) {
    return B > 0 && T >= 1 && T <= OE_RNNT_MAX_T && Umax >= 0 && Umax <= OE_RNNT_MAX_U && B * T * (Umax + 1) < (1L << 31);
}

extern "C" size_t oe_rnnt_workspace_bytes(int B, int T, int Umax) {
    if (!rt_shape_ok(B, T, Umax)) return 0;
    const size_t N = (size_t)B * (size_t)T * ((size_t)Umax + 1);
    return 3 * rt_up16(4 * N) + 2 * rt_up16(8 * N) + rt_up16(8 * (size_t)B) + rt_up16(4 * (size_t)B);
}

static RtWs rt_carve(void* workspace, int B, int T, int Umax) {
    const size_t N = (size_t)B * (size_t)T * ((size_t)Umax + 1);
    char* p = reinterpret_cast<char*>(workspace);
    RtWs w;
    w.lse = reinterpret_cast<float*>(p); p += rt_up16(4 * N);
    w.lpb = reinterpret_cast<float*>(p); p += rt_up16(4 * N);
    w.lpl = reinterpret_cast<float*>(p); p += rt_up16(4 * N);
    w.alpha = reinterpret_cast<double*>(p); p += rt_up16(8 * N);
    w.beta = reinterpret_cast<double*>(p); p += rt_up16(8 * N);
    w.logz = reinterpret_cast<double*>(p); p += rt_up16(8 * (size_t)B);
    w.status = reinterpret_cast<int*>(p);
    return w;
}

// the checks the two entries share; everything is reported before any launch
static int rt_check(const char* name, const float* logits, long ldv, int B, int T, int Umax, int V, const int* hlens, const int* targets,
                    const int* ulens, int blank, void* workspace) {
    OE_REQUIRE(logits, "%s: null logits", name);
    OE_REQUIRE(hlens && ulens, "%s: null hlens / ulens", name);
    OE_REQUIRE(workspace, "%s: null workspace", name);
    OE_REQUIRE(B > 0 && T >= 1 && T <= OE_RNNT_MAX_T, "%s: bad shape B=%d T=%d (1 <= B, 1 <= T <= %d)", name, B, T, OE_RNNT_MAX_T);
    OE_REQUIRE(Umax >= 0 && Umax <= OE_RNNT_MAX_U, "%s: Umax=%d outside 0 .. %d (a lane holds at most 4 label positions)", name, Umax,
               OE_RNNT_MAX_U);
    OE_REQUIRE(V >= 2 && ldv >= V, "%s: V=%d ldv=%ld (2 <= V, ldv >= V)", name, V, ldv);
    OE_REQUIRE(blank >= 0 && blank < V, "%s: blank=%d outside 0 .. V-1 = %d", name, blank, V - 1);
    OE_REQUIRE(targets || Umax == 0, "%s: null targets with Umax=%d", name, Umax);
    OE_REQUIRE((long)B * T * (Umax + 1) < (1L << 31), "%s: B*T*(Umax+1) = %ld nodes, the limit is 2^31 - 1", name, (long)B * T * (Umax + 1));
    OE_REQUIRE((((uintptr_t)workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", name);
    return 0;
}

extern "C" int oe_rnnt_loss(const oe_rnnt_args* args, void* stream) {
    OE_REQUIRE(args, "oe_rnnt_loss: null args");
    const oe_rnnt_args& a = *args;
    if (int rc = rt_check("oe_rnnt_loss", a.logits, a.ldv, a.B, a.T, a.Umax, a.V, a.hlens, a.targets, a.ulens, a.blank, a.workspace)) return rc;
    OE_REQUIRE(a.logp, "oe_rnnt_loss: null logp");
    hipStream_t st = (hipStream_t)stream;
    const RtWs w = rt_carve(a.workspace, a.B, a.T, a.Umax);
    const int U1 = a.Umax + 1;
    const long nodes = (long)a.B * a.T * U1;
    hipLaunchKernelGGL(rt_rows_kernel, dim3(oe_cdiv(nodes, 4)), dim3(256), 0, st, a.logits, a.ldv, nodes, a.T, U1, a.V, a.hlens, a.targets,
                       a.ulens, a.blank, w);
    OE_LAUNCH_CHECK("rnnt_rows");
#define RT_LATTICE(NS)                                                                                                              \
    hipLaunchKernelGGL(rt_lattice_kernel<NS>, dim3((unsigned)a.B), dim3(128), 0, st, a.T, U1, a.V, a.hlens, a.targets, a.ulens, a.blank, \
                       a.logp, a.status, w)
    if (U1 <= 64) RT_LATTICE(1);
    else if (U1 <= 128) RT_LATTICE(2);
    else RT_LATTICE(4);
#undef RT_LATTICE
    OE_LAUNCH_CHECK("rnnt_lattice");
    return 0;
}

extern "C" int oe_rnnt_grad(const oe_rnnt_grad_args* args, void* stream) {
    OE_REQUIRE(args, "oe_rnnt_grad: null args");
    const oe_rnnt_grad_args& a = *args;
    if (int rc = rt_check("oe_rnnt_grad", a.logits, a.ldv, a.B, a.T, a.Umax, a.V, a.hlens, a.targets, a.ulens, a.blank, a.workspace)) return rc;
    OE_REQUIRE(a.g && a.dlogits, "oe_rnnt_grad: null pointer (g / dlogits)");
    hipStream_t st = (hipStream_t)stream;
    const RtWs w = rt_carve(a.workspace, a.B, a.T, a.Umax);
    const int U1 = a.Umax + 1;
    const long nodes = (long)a.B * a.T * U1;
    hipLaunchKernelGGL(rt_grad_kernel, dim3(oe_cdiv(nodes, 4)), dim3(256), 0, st, a.logits, a.ldv, nodes, a.T, U1, a.V, a.hlens, a.targets,
                       a.ulens, a.blank, a.g, a.dlogits, w);
    OE_LAUNCH_CHECK("rnnt_grad");
    return 0;
}

static int jc_check(const char* name, const float* e, const float* p, int B, int T, int U1, int J, int act) {
    OE_REQUIRE(e && p, "%s: null e / p", name);
    OE_REQUIRE(B > 0 && T > 0 && U1 > 0 && J > 0 && (long)B * T * U1 < (1L << 31), "%s: bad shape B=%d T=%d U1=%d J=%d", name, B, T, U1, J);
    OE_REQUIRE(act >= OE_ACT_NONE && act <= OE_ACT_GELU, "%s: unknown act=%d", name, act);
    return 0;
}

extern "C" int oe_joint_combine_fwd(const oe_joint_combine_args* args, void* stream) {
    OE_REQUIRE(args, "oe_joint_combine_fwd: null args");
    const oe_joint_combine_args& a = *args;
    if (int rc = jc_check("oe_joint_combine_fwd", a.e, a.p, a.B, a.T, a.U1, a.J, a.act)) return rc;
    OE_REQUIRE(a.z, "oe_joint_combine_fwd: null z");
    hipLaunchKernelGGL(jc_fwd_kernel, dim3((unsigned)((long)a.B * a.T)), dim3(256), 0, (hipStream_t)stream, a.e, a.p, a.T, a.U1, a.J, a.act,
                       a.hlens, a.ulens, a.z);
    OE_LAUNCH_CHECK("joint_combine_fwd");
    return 0;
}

extern "C" int oe_joint_combine_bwd(const oe_joint_combine_bwd_args* args, void* stream) {
    OE_REQUIRE(args, "oe_joint_combine_bwd: null args");
    const oe_joint_combine_bwd_args& a = *args;
    if (int rc = jc_check("oe_joint_combine_bwd", a.e, a.p, a.B, a.T, a.U1, a.J, a.act)) return rc;
    OE_REQUIRE(a.dz && a.de && a.dp, "oe_joint_combine_bwd: null dz / de / dp");
    hipLaunchKernelGGL(jc_bwd_kernel, dim3((unsigned)((long)a.B * a.T + (long)a.B * a.U1)), dim3(256), 0, (hipStream_t)stream, a.e, a.p, a.B,
                       a.T, a.U1, a.J, a.act, a.hlens, a.ulens, a.dz, a.de, a.dp);
    OE_LAUNCH_CHECK("joint_combine_bwd");
    return 0;
}
