// Grammar-constrained CTC decoding: the best path of the CTC posteriors through an epsilon-free weighted token graph, the CTC
// topology (blank, repeats) applied implicitly.  The semantics every layer refers to are in include/openeat_hip.h
// (oe_ctc_graph); the tie rule is oe_ctc_align's, generalised.
//
// Per utterance there is a value per node (n: last frame blank) and per arc (r: last frame emitted the arc's label).  Two launches:
//   launch 1  lp_rows_kernel (lp_rows.hip): the blank and the U label columns of every frame as lp, a compact row of U + 1 floats.
//   launch 2  graph_kernel: ONE WORKGROUP of 1024 threads PER UTTERANCE, the state values in LDS.  A frame is two phases
//             with a barrier behind each:
//             A  per node q, over its incoming arcs (they are contiguous: arcs are sorted by dst): the best r, lowest id on
//                ties, with its label (v1, id1, c1), and the best r whose label differs from c1 (v2, id2).  With
//                n' = n_{t-1}[q]:  m1 = best(n', v1), m2 = best(n', v2), n' kept unless the arc is strictly greater.  Nodes of
//                in-degree <= 32 take a thread each; the others (a token loop: one node, V - 1 arcs) a wave each, a lane per
//                64th arc and a two-best merge across the wave.  n itself is not stored: n_t[q] = lp[t,0] + m1_t[q].
//             B  per arc a: r_t[a] = lp[t,label] + best(r_{t-1}[a], (c1[src] != label ? m1[src] : m2[src]) + w[a]) - the
//                max over "the node, then every incoming arc of another label" from two values, O(A + Q) per frame.  The
//                weight is added to the maximum, not to every candidate: the same winner wherever the sums are exact, and
//                elsewhere a tie between the node and an arc that only the rounding of + w creates goes to the arc.
//             LDS: 4 bytes per arc (r) and 12 per node (m1, m2, c1): 4 * 16384 + 12 * 8064 + 1.2 KB of lists and
//             reduction slots <= 160 KiB, which is where the limits come from.  Where 4 more bytes per arc fit in the same
//             budget (graph_kernel<true>) the arcs' columns are kept there too and phase A reads only in_ptr from L2.
//             Back-pointers: per frame a word per node (id1, id2 in 15 bits each, "m1 is the arc", "m2 is the arc") and a
//             byte per arc (stay / through m1 / through m2), written as they are made, read by the back-trace only.
//             Then: the end state by a workgroup arg-max (lowest index on ties: nodes, then arcs), the back-trace by one
//             thread (a chain of Tb dependent loads), and the traversal list by all threads (a ballot scan of the starts;
//             the thread of a start walks to the traversal's end, summing lp in frame order).
//             The first arc of every thread (a < 1024) keeps src / label / weight in registers and has its lp of frame t + 1
//             loaded during frame t (GRAPH_PF = 1); the arcs behind it read theirs from L2 inside phase B.
// No workgroup waits for another, no float atomics, no allocation, no host read: capturable.
#include <stdlib.h>
#include "ctc_graph_common.h"
#include "../../include/openeat_hip.h"

#define GRAPH_BLOCK 1024
#define GRAPH_WAVES (GRAPH_BLOCK / 64)
#define GRAPH_PF 1                                // frames of lp in flight ahead of the recursion (a thread's first arc)
#define GRAPH_MAX_A OE_CTC_GRAPH_MAX_ARCS
#define GRAPH_MAX_Q OE_CTC_GRAPH_MAX_NODES
#define GRAPH_HEAVY 32                            // a node of more incoming arcs than this takes a wave, not a thread
#define GRAPH_MAX_HEAVY (GRAPH_MAX_A / (GRAPH_HEAVY + 1) + 1)
#define GRAPH_NONE 0x7fffffff                     // "no arc" (0x7fff in a back-pointer word)

static_assert(4 * GRAPH_MAX_A + 12 * GRAPH_MAX_Q + 2 * GRAPH_MAX_HEAVY + 512 <= 160 * 1024, "oe_ctc_graph: the limits exceed the LDS");
static_assert(GRAPH_MAX_A <= 0x7fff, "oe_ctc_graph: an arc id and 'none' must fit 15 bits of a back-pointer word");

// ---------------------------------------------------------------- launch 2 ----
struct GraphParams {
    const float* cw; unsigned* bp; long bp_stride;                            // bp_stride: words per frame = Q + ceil(A / 4)
    int T, U, Q, A, max_trav;
    const int* hlens; const int* in_ptr; const int* src; const int* dst; const int* label; const int* col;
    const float* w; const float* fin;
    float* score; int* frames; int* arcs; float* path_logp;
    int* n_trav; int* trav_arc; int* trav_start; int* trav_end; float* trav_logp;
};

// The two best of a set of incoming arcs: (v1, id1, c1) the best, lowest id on ties, and its label; (v2, id2) the best among
// the arcs whose label is not c1.  An unreachable arc (-inf) never enters: "none" is (-inf, GRAPH_NONE, -1).
struct TwoBest { float v1; int id1, c1; float v2; int id2; };

// arcs arrive by ascending id: strictly greater replaces
__device__ __forceinline__ void graph_push(TwoBest& s, float v, int id, int c) {
    if (v > s.v1) {
        if (c != s.c1) { s.v2 = s.v1; s.id2 = s.id1; }                        // the old best is the best of another label now
        s.v1 = v; s.id1 = id; s.c1 = c;
    } else if (c != s.c1 && v > s.v2) {
        s.v2 = v; s.id2 = id;
    }
}

__device__ __forceinline__ TwoBest graph_merge(const TwoBest& x, const TwoBest& y) {
    const bool xw = graph_better(x.v1, x.id1, y.v1, y.id1);
    TwoBest w, l;                                                            // winner, loser: selects field by field, all in registers
    w.v1 = xw ? x.v1 : y.v1; w.id1 = xw ? x.id1 : y.id1; w.c1 = xw ? x.c1 : y.c1; w.v2 = xw ? x.v2 : y.v2; w.id2 = xw ? x.id2 : y.id2;
    l.v1 = xw ? y.v1 : x.v1; l.id1 = xw ? y.id1 : x.id1; l.c1 = xw ? y.c1 : x.c1; l.v2 = xw ? y.v2 : x.v2; l.id2 = xw ? y.id2 : x.id2;
    const bool same = l.c1 == w.c1;
    const float lv = same ? l.v2 : l.v1;                                     // the loser's best of a label other than the winner's
    const int li = same ? l.id2 : l.id1;
    if (graph_better(lv, li, w.v2, w.id2)) { w.v2 = lv; w.id2 = li; }
    return w;
}

// COLS: the arcs' columns are also kept in LDS (4 more bytes per arc, where they fit): phase A then reads no global memory but in_ptr
template <bool COLS>
__global__ __launch_bounds__(GRAPH_BLOCK) void graph_kernel(const GraphParams p) {
    extern __shared__ __attribute__((aligned(16))) float graph_sh[];
    __shared__ unsigned short heavy[GRAPH_MAX_HEAVY];
    __shared__ int n_heavy;
    __shared__ float red_v[GRAPH_WAVES];
    __shared__ int red_i[GRAPH_WAVES];
    __shared__ int end_state;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int T = p.T, U = p.U, Q = p.Q, A = p.A, max_trav = p.max_trav;
    float* r = graph_sh;
    float* m1 = r + A;
    float* m2 = m1 + Q;
    int* c1 = reinterpret_cast<int*>(m2 + Q);
    int* colc = c1 + Q;                                                      // COLS only
    const int Tb = max(min(p.hlens[b], T), 0);
    const long rw = U + 1;
    const float* cw = p.cw + (long)b * T * rw;
    unsigned* bp = p.bp + (long)b * T * p.bp_stride;
    int* frames = p.frames + (long)b * T;
    int* arcs = p.arcs + (long)b * T;
    float* path_logp = p.path_logp ? p.path_logp + (long)b * T : nullptr;

    // ---- before frame 0: n[0] = 0 (kept as m1 with a zero lp), everything else unreachable; the list of wide nodes
    for (int a = tid; a < A; a += GRAPH_BLOCK) {
        r[a] = -INFINITY;
        if (COLS) colc[a] = min(max(p.col[a], 0), U - 1);
    }
    for (int q = tid; q < Q; q += GRAPH_BLOCK) m1[q] = q == 0 ? 0.f : -INFINITY;
    if (tid == 0) n_heavy = 0;
    __syncthreads();
    for (int q = tid; q < Q; q += GRAPH_BLOCK) {
        const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
        if (hi - lo > GRAPH_HEAVY) {
            const int i = atomicAdd(&n_heavy, 1);                            // the order of the list does not reach the results
            if (i < GRAPH_MAX_HEAVY) heavy[i] = (unsigned short)q;
        }
    }
    __syncthreads();
    const int nh = min(n_heavy, GRAPH_MAX_HEAVY);

    // the thread's first arc: its constants in registers, its lp a frame ahead
    const bool has0 = tid < A;
    int s0 = 0, k0 = 0;
    float w0 = 0.f, lp_next = 0.f;
    if (has0) {
        s0 = min(max(p.src[tid], 0), Q - 1);
        k0 = min(max(p.col[tid], 0), U - 1);
        w0 = p.w[tid];
        if (Tb > 0) lp_next = cw[1 + k0];
    }

    float lp0_prev = 0.f;
    for (int t = 0; t < Tb; ++t) {
        const float* row = cw + (long)t * rw;
        const float lp0 = row[0];
        const float lp_a0 = lp_next;
        if (has0 && t + GRAPH_PF < Tb) lp_next = row[rw + 1 + k0];
        unsigned* wn = bp + (long)t * p.bp_stride;
        unsigned char* wa = reinterpret_cast<unsigned char*>(wn + Q);

        // ---- phase A: per node, the two best incoming arcs of frame t-1
        auto col_of = [&](int a) { return COLS ? colc[a] : min(max(p.col[a], 0), U - 1); };
        auto node_done = [&](int q, const TwoBest& s) {
            const float np = lp0_prev + m1[q];                                // n_{t-1}[q]
            float M1 = np, M2 = np;
            unsigned f = 0;
            if (s.v1 > M1) { M1 = s.v1; f |= 1u << 30; }
            if (s.v2 > M2) { M2 = s.v2; f |= 1u << 31; }
            m1[q] = M1; m2[q] = M2; c1[q] = s.c1;
            wn[q] = (unsigned)(s.id1 & 0x7fff) | ((unsigned)(s.id2 & 0x7fff) << 15) | f;
        };
        for (int q = tid; q < Q; q += GRAPH_BLOCK) {
            const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
            if (hi - lo > GRAPH_HEAVY) continue;
            TwoBest s = {-INFINITY, GRAPH_NONE, -1, -INFINITY, GRAPH_NONE};
            for (int a = lo; a < hi; ++a) graph_push(s, r[a], a, col_of(a));
            node_done(q, s);
        }
        for (int i = wave; i < nh; i += GRAPH_WAVES) {
            const int q = heavy[i];
            const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
            TwoBest s = {-INFINITY, GRAPH_NONE, -1, -INFINITY, GRAPH_NONE};
            for (int a = lo + lane; a < hi; a += 64) graph_push(s, r[a], a, col_of(a));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                TwoBest y;
                y.v1 = __shfl_xor(s.v1, o, 64); y.id1 = __shfl_xor(s.id1, o, 64); y.c1 = __shfl_xor(s.c1, o, 64);
                y.v2 = __shfl_xor(s.v2, o, 64); y.id2 = __shfl_xor(s.id2, o, 64);
                s = graph_merge(s, y);
            }
            if (lane == 0) node_done(q, s);
        }
        __syncthreads();

        // ---- phase B: per arc
        for (int a = tid; a < A; a += GRAPH_BLOCK) {
            int s, k;
            float w, lp;
            if (a == tid) { s = s0; k = k0; w = w0; lp = lp_a0; }
            else {
                s = min(max(p.src[a], 0), Q - 1);
                k = min(max(p.col[a], 0), U - 1);
                w = p.w[a];
                lp = row[1 + k];
            }
            const bool other = c1[s] != k;
            const float cand = (other ? m1[s] : m2[s]) + w;
            float best = r[a];
            unsigned char code = 0;
            if (cand > best) { best = cand; code = other ? 1 : 2; }
            r[a] = lp + best;
            wa[a] = code;
        }
        __syncthreads();
        lp0_prev = lp0;
    }

    // ---- the end: nodes by ascending q, then arcs by ascending id; a later one only if strictly greater
    float bv = -INFINITY;
    int bi = GRAPH_NONE;
    if (Tb > 0) {
        for (int q = tid; q < Q; q += GRAPH_BLOCK) {
            const float v = (lp0_prev + m1[q]) + p.fin[q];
            if (v > bv) { bv = v; bi = q; }
        }
        for (int a = tid; a < A; a += GRAPH_BLOCK) {
            const float v = r[a] + p.fin[min(max(p.dst[a], 0), Q - 1)];
            if (v > bv) { bv = v; bi = Q + a; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(bv, o, 64);
        const int i = __shfl_xor(bi, o, 64);
        if (graph_better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < GRAPH_WAVES; ++i)
            if (graph_better(red_v[i], red_i[i], bv, bi)) { bv = red_v[i]; bi = red_i[i]; }
        const bool ok = bv > -INFINITY;
        end_state = ok ? bi : -1;
        p.score[b] = ok ? bv : -INFINITY;
        // ---- back-trace: cur < Q a node state, else the arc state cur - Q
        if (ok) {
            int cur = bi, a = -1, lab = 0, k = 0, s = 0;
            for (int t = Tb - 1; t >= 0; --t) {
                const unsigned* wn = bp + (long)t * p.bp_stride;
                if (cur >= Q) {
                    if (cur - Q != a) {
                        a = cur - Q;
                        lab = p.label[a];
                        k = min(max(p.col[a], 0), U - 1);
                        s = min(max(p.src[a], 0), Q - 1);
                    }
                    frames[t] = lab;
                    arcs[t] = a;
                    if (path_logp) path_logp[t] = cw[(long)t * rw + 1 + k];
                    const unsigned code = reinterpret_cast<const unsigned char*>(wn + Q)[a];
                    if (code) {
                        const unsigned word = wn[s];
                        const bool arc = code == 1 ? (word >> 30) & 1 : word >> 31;
                        const int id = code == 1 ? word & 0x7fff : (word >> 15) & 0x7fff;
                        cur = arc ? Q + min(id, A - 1) : s;
                    }
                } else {
                    frames[t] = 0;
                    arcs[t] = -1;
                    if (path_logp) path_logp[t] = cw[(long)t * rw];
                    const unsigned word = wn[cur];
                    if ((word >> 30) & 1) cur = Q + min((int)(word & 0x7fff), A - 1);
                }
            }
        }
    }
    __syncthreads();
    const bool ok = end_state >= 0;
    for (int t = (ok ? Tb : 0) + tid; t < T; t += GRAPH_BLOCK) {
        frames[t] = -1;
        arcs[t] = -1;
        if (path_logp) path_logp[t] = 0.f;
    }

    // ---- traversals: a start at t iff arcs[t] >= 0 and (t == 0 or arcs[t-1] != arcs[t]); slots in frame order
    int* ta = p.trav_arc + (long)b * max_trav;
    int* ts = p.trav_start + (long)b * max_trav;
    int* te = p.trav_end + (long)b * max_trav;
    float* tl = p.trav_logp ? p.trav_logp + (long)b * max_trav : nullptr;
    int count = 0;
    if (ok) {
        for (int c0 = 0; c0 < Tb; c0 += GRAPH_BLOCK) {
            const int t = c0 + tid;
            const int a = t < Tb ? arcs[t] : -1;
            const bool start = a >= 0 && (t == 0 || arcs[t - 1] != a);
            const unsigned long long m = __ballot(start);
            if (lane == 0) red_i[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
            for (int i = 0; i < GRAPH_WAVES; ++i) {
                const int n = red_i[i];
                if (i < wave) before += n;
                total += n;
            }
            const int slot = count + before + __popcll(m & ((1ull << lane) - 1ull));
            if (start && slot < max_trav) {
                const int k = min(max(p.col[a], 0), U - 1);
                int e = t;
                float sum = cw[(long)t * rw + 1 + k];
                while (e + 1 < Tb && arcs[e + 1] == a) {
                    ++e;
                    sum += cw[(long)e * rw + 1 + k];
                }
                ta[slot] = a; ts[slot] = t; te[slot] = e;
                if (tl) tl[slot] = sum;
            }
            count += total;
            __syncthreads();
        }
    }
    for (int i = min(count, max_trav) + tid; i < max_trav; i += GRAPH_BLOCK) {
        ta[i] = -1; ts[i] = -1; te[i] = -1;
        if (tl) tl[i] = 0.f;
    }
    if (tid == 0) p.n_trav[b] = count;
}

// ---------------------------------------------------------------- host -------
static bool graph_shape_ok(long B, long T, long U, long Q, long A) {
    return B > 0 && T > 0 && T <= GRAPH_MAX_T && U > 0 && Q >= 1 && Q <= GRAPH_MAX_Q && A >= 1 && A <= GRAPH_MAX_A;
}
static size_t graph_bp_stride(int Q, int A) { return (size_t)Q + ((size_t)A + 3) / 4; }

extern "C" size_t oe_ctc_graph_workspace_bytes(int B, int T, int U, int Q, int A) {
    if (!graph_shape_ok(B, T, U, Q, A)) return 0;
    return (size_t)B * (size_t)T * (((size_t)U + 1) + graph_bp_stride(Q, A)) * 4;
}

extern "C" int oe_ctc_graph(const oe_ctc_graph_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph: null args");
    const oe_ctc_graph_args& a = *args;
    if (int rc = graph_check("oe_ctc_graph", a.graph, a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.workspace, &a.max_trav)) return rc;
    const oe_decoding_graph& g = *a.graph;
    OE_REQUIRE(a.score && a.frames && a.arcs && a.n_trav && a.trav_arc && a.trav_start && a.trav_end,
               "oe_ctc_graph: null output (score, frames, arcs, n_trav, trav_arc, trav_start, trav_end)");
    OE_REQUIRE(g.Q >= 1 && g.Q <= GRAPH_MAX_Q, "oe_ctc_graph: Q=%d nodes outside 1 .. %d (the node values live in LDS)", g.Q, GRAPH_MAX_Q);
    OE_REQUIRE(g.A >= 1 && g.A <= GRAPH_MAX_A, "oe_ctc_graph: A=%d arcs outside 1 .. %d (the arc values live in LDS)", g.A, GRAPH_MAX_A);
    OE_REQUIRE(g.in_ptr && g.src && g.dst && g.label && g.col && g.w && g.final && g.cols,
               "oe_ctc_graph: null table in graph (in_ptr, src, dst, label, col, w, final, cols)");
    const size_t lds_max = 4 * (size_t)GRAPH_MAX_A + 12 * (size_t)GRAPH_MAX_Q;
    const bool cols_in_lds = 8 * (size_t)g.A + 12 * (size_t)g.Q <= lds_max;
    const size_t lds = (cols_in_lds ? 8 : 4) * (size_t)g.A + 12 * (size_t)g.Q;
    if (lds > 48 * 1024) {
        static bool raised = false;                                   // once per process: opt in to more than 64 KB of dynamic LDS
        if (!raised) {
            if (hipFuncSetAttribute((const void*)graph_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess ||
                hipFuncSetAttribute((const void*)graph_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess) {
                oe_set_error("oe_ctc_graph: cannot raise the dynamic LDS limit");
                return -1;
            }
            raised = true;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    float* cw = reinterpret_cast<float*>(a.workspace);
    const long rows = (long)a.B * a.T;
    if (int rc = oe_lp_rows("oe_ctc_graph", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, g.cols, g.U, a.normalized, cw, nullptr, st))
        return rc;
    GraphParams p;
    p.cw = cw;
    p.bp = reinterpret_cast<unsigned*>(cw + rows * ((long)g.U + 1));
    p.bp_stride = (long)graph_bp_stride(g.Q, g.A);
    p.T = a.T; p.U = g.U; p.Q = g.Q; p.A = g.A; p.max_trav = a.max_trav;
    p.hlens = a.hlens; p.in_ptr = g.in_ptr; p.src = g.src; p.dst = g.dst; p.label = g.label; p.col = g.col; p.w = g.w; p.fin = g.final;
    p.score = a.score; p.frames = a.frames; p.arcs = a.arcs; p.path_logp = a.path_logp;
    p.n_trav = a.n_trav; p.trav_arc = a.trav_arc; p.trav_start = a.trav_start; p.trav_end = a.trav_end; p.trav_logp = a.trav_logp;
    if (cols_in_lds) hipLaunchKernelGGL(graph_kernel<true>, dim3((unsigned)a.B), dim3(GRAPH_BLOCK), lds, st, p);
    else hipLaunchKernelGGL(graph_kernel<false>, dim3((unsigned)a.B), dim3(GRAPH_BLOCK), lds, st, p);
    OE_LAUNCH_CHECK("ctc_graph");
    return 0;
}
