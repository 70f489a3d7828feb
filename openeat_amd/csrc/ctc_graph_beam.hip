// Beam-pruned CTC decoding over large token graphs: oe_ctc_graph's recursion by token passing.  The semantics every layer refers
// to are in include/openeat_hip.h (oe_ctc_graph_beam); the arithmetic, the tie rule and the end rule are ctc_graph.hip's.
//
// Two launches:
//   launch 1  lp_rows_kernel (lp_rows.hip): the blank and the U label columns of every frame as lp, a compact row of U + 1 floats.
//   launch 2  beam_kernel: ONE WORKGROUP of 1024 threads PER UTTERANCE, the state in global memory.
// Per utterance, dense and paid once (the stamps and keys are zeroed before frame 0, everything else is guarded by a stamp):
//   per arc   rv value, rs stamp, rpos position in the list it is alive in;
//   per node  nv, ns, npos likewise; tstamp "touched in frame t"; key1, key2 the 64-bit push keys;
//   cand      Q + A slots (state id, back-pointer): the states a frame makes, before pruning.
// A stamp s says "alive as input of frame s - 1" (0: never), so a frame's values need no reset: they expire.  L_t, the list of
// the states alive as input of frame t (L_0 = {node 0}), holds per entry the state id (q, or Q + a) and the position in
// L_{t-1} of its predecessor; lists are appended to through an LDS counter, a wave's entries in one add, so positions are in
// no fixed order - and they reach no output: a back-pointer is followed, never compared.  Frame t, a barrier behind each step:
//   1  every entry of L_t touches a node (itself, or its arc's dst): the first toucher (atomicMax on tstamp) appends it to the
//      touched list; an arc pushes (value, inverted id) to key1[dst] by a 64-bit atomicMax: v1 / id1, lowest id on ties.
//   2  every arc of L_t whose label is not that of id1 pushes to key2[dst]: v2 / id2.
//   3a per touched node: m1, m2, c1 and the list positions behind them, kept by position in the touched list; the keys are
//      reset here, by walking the list; n_t[q] = lp0 + m1 is made and q becomes a candidate.  A node of more than 16 leaving
//      arcs goes on the wide list.
//   3b the arcs leaving the touched nodes (out_ptr / out_arc): r_t[a] as ctc_graph.hip's phase B.  A thread per node, a wave
//      per wide node.  An arc has one src, so it is made once.
//   4  the arcs of L_t that 3b did not reach (their src has no alive state): stay.
//   5  best_t by a workgroup maximum; thr_t = best_t - beam, -inf on the last frame.
//   6  the candidates at or above thr_t are appended to L_{t+1} and learn their position; the others get stamp 0.  More than
//      max_active of them: overflow, with the count.
// Work per frame: O(|L_t| + the arcs leaving the touched nodes).  Then the end rule by an arg-max over the last list (ties: the
// lowest state id, which is oe_ctc_graph's order), the back-trace by one thread along the positions, and ctc_graph.hip's
// traversal list.
// Values written by an atomic (keys, tstamp) are read by atomic loads; everything else is written and read by the waves of
// one workgroup with a barrier between.  No workgroup waits for another, no float atomics, no allocation, no host read.
#include <stdlib.h>
#include "ctc_graph_common.h"
#include "../../include/openeat_hip.h"

#define BEAM_BLOCK 1024
#define BEAM_WAVES (BEAM_BLOCK / 64)
#define BEAM_MAX_T GRAPH_MAX_T
#define BEAM_MAX_Q OE_CTC_GRAPH_BEAM_MAX_NODES
#define BEAM_MAX_A OE_CTC_GRAPH_BEAM_MAX_ARCS
#define BEAM_WIDE 16                              // a node of more leaving arcs than this takes a wave, not a thread
#define BEAM_NONE 0x7fffffff

// ---------------------------------------------------------------- launch 2 ----
// The per-utterance workspace: byte offsets of its parts, every one a multiple of 16 (Q, A, M are rounded up to 4).
struct BeamLayout {
    size_t key1, key2, rs, ns, tstamp, nv, npos, rv, rpos, cand, touched, wide, tm1, tm2, tc1, tp1, tp2, rec, bytes;
    size_t zero_bytes;                                                        // key1 .. tstamp: zeroed before frame 0
    long Mp;
};
static BeamLayout beam_layout(long T, long Q, long A, long M) {
    const size_t Qp = (size_t)(Q + 3) & ~(size_t)3, Ap = (size_t)(A + 3) & ~(size_t)3, Mp = (size_t)(M + 3) & ~(size_t)3;
    BeamLayout l;
    size_t o = 0;
    l.key1 = o; o += 8 * Qp;
    l.key2 = o; o += 8 * Qp;
    l.rs = o; o += 4 * Ap;
    l.ns = o; o += 4 * Qp;
    l.tstamp = o; o += 4 * Qp;
    l.zero_bytes = o;
    l.nv = o; o += 4 * Qp;
    l.npos = o; o += 4 * Qp;
    l.rv = o; o += 4 * Ap;
    l.rpos = o; o += 4 * Ap;
    l.cand = o; o += 8 * (Qp + Ap);
    l.touched = o; o += 4 * Mp;
    l.wide = o; o += 4 * Mp;
    l.tm1 = o; o += 4 * Mp;
    l.tm2 = o; o += 4 * Mp;
    l.tc1 = o; o += 4 * Mp;
    l.tp1 = o; o += 4 * Mp;
    l.tp2 = o; o += 4 * Mp;
    l.rec = o; o += 8 * (size_t)T * Mp;
    l.bytes = o;                                                              // 40 Q' + 20 A' + 28 M' + 8 T M'
    l.Mp = (long)Mp;
    return l;
}

struct BeamParams {
    const float* cw; char* ws; BeamLayout l;
    int T, U, Q, A, M, max_active, max_trav;
    float beam;
    const int* hlens; const int* dst; const int* label; const int* col; const float* w; const float* fin;
    const int* out_ptr; const int* out_arc;
    float* score; int* frames; int* arcs; float* path_logp;
    int* n_trav; int* trav_arc; int* trav_start; int* trav_end; float* trav_logp;
    int* status; int* peak;
};

__global__ __launch_bounds__(BEAM_BLOCK) void beam_kernel(const BeamParams p) {
    __shared__ int s_ntouched, s_nwide, s_ncand, s_nsurv;
    __shared__ float red_v[BEAM_WAVES];
    __shared__ int red_i[BEAM_WAVES], red_p[BEAM_WAVES];
    __shared__ int end_state;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int T = p.T, U = p.U, Q = p.Q, A = p.A, M = p.M, max_trav = p.max_trav;
    const int QA = Q + A;
    const long Mp = p.l.Mp;
    char* ws = p.ws + (size_t)b * p.l.bytes;
    beam_u64* key1 = reinterpret_cast<beam_u64*>(ws + p.l.key1);
    beam_u64* key2 = reinterpret_cast<beam_u64*>(ws + p.l.key2);
    int* rs = reinterpret_cast<int*>(ws + p.l.rs);
    int* ns = reinterpret_cast<int*>(ws + p.l.ns);
    int* tstamp = reinterpret_cast<int*>(ws + p.l.tstamp);
    float* nv = reinterpret_cast<float*>(ws + p.l.nv);
    int* npos = reinterpret_cast<int*>(ws + p.l.npos);
    float* rv = reinterpret_cast<float*>(ws + p.l.rv);
    int* rpos = reinterpret_cast<int*>(ws + p.l.rpos);
    int2* cand = reinterpret_cast<int2*>(ws + p.l.cand);
    int* touched = reinterpret_cast<int*>(ws + p.l.touched);
    int* wide = reinterpret_cast<int*>(ws + p.l.wide);
    float* tm1 = reinterpret_cast<float*>(ws + p.l.tm1);
    float* tm2 = reinterpret_cast<float*>(ws + p.l.tm2);
    int* tc1 = reinterpret_cast<int*>(ws + p.l.tc1);
    int* tp1 = reinterpret_cast<int*>(ws + p.l.tp1);
    int* tp2 = reinterpret_cast<int*>(ws + p.l.tp2);
    int2* rec = reinterpret_cast<int2*>(ws + p.l.rec);
    const int Tb = max(min(p.hlens[b], T), 0);
    const long rw = U + 1;
    const float* cw = p.cw + (long)b * T * rw;
    int* frames = p.frames + (long)b * T;
    int* arcs = p.arcs + (long)b * T;
    float* path_logp = p.path_logp ? p.path_logp + (long)b * T : nullptr;
    auto col_of = [&](int a) { return min(max(p.col[a], 0), U - 1); };
    auto dst_of = [&](int a) { return min(max(p.dst[a], 0), Q - 1); };

    // ---- before frame 0: the one sweep over the graph's size; n[0] = 0 is alive as input of frame 0
    {
        int4* z = reinterpret_cast<int4*>(ws);
        const size_t nz = p.l.zero_bytes / 16;
        for (size_t i = tid; i < nz; i += BEAM_BLOCK) z[i] = make_int4(0, 0, 0, 0);
    }
    if (tid == 0) { s_ntouched = 0; s_nwide = 0; s_ncand = 0; s_nsurv = 0; }
    __syncthreads();
    if (tid == 0) { nv[0] = 0.f; ns[0] = 1; npos[0] = 0; }
    __syncthreads();

    int n = Tb > 0 ? 1 : 0;                                                  // |L_t|
    int peak = 0, status = OE_CTC_GRAPH_BEAM_OK, done = 0;
    for (int t = 0; t < Tb; ++t) {
        const int2* Lin = rec + (size_t)max(t - 1, 0) * Mp;                   // L_t (t >= 1); L_0 = {node 0} is not stored
        int2* Lout = rec + (size_t)t * Mp;                                    // L_{t+1}
        const int tag_in = t + 1, tag_out = t + 2;
        const float* row = cw + (long)t * rw;
        const float lp0 = row[0];
        float lmax = -INFINITY;

        // ---- 1: touch, push v1
        for (int base = 0; base < n; base += BEAM_BLOCK) {
            const int i = base + tid;
            const bool valid = i < n;
            bool first = false;
            int d = 0;
            if (valid) {
                const int c = t ? Lin[i].x : 0;
                if (c < Q) d = c;
                else {
                    const int a = c - Q;
                    d = dst_of(a);
                    atomicMax(&key1[d], beam_key(rv[a], a));
                }
                first = atomicMax(&tstamp[d], tag_in) != tag_in;
            }
            const int j = beam_append(&s_ntouched, first);
            if (first && j < M) touched[j] = d;
        }
        __syncthreads();
        if (tid == 0) { s_ncand = 0; s_nsurv = 0; }

        // ---- 2: push v2, the best of a label other than id1's
        for (int i = tid; i < n; i += BEAM_BLOCK) {
            const int c = t ? Lin[i].x : 0;
            if (c < Q) continue;
            const int a = c - Q, d = dst_of(a);
            const int id1 = min(max(beam_key_id(beam_load(&key1[d])), 0), A - 1);
            if (col_of(a) != col_of(id1)) atomicMax(&key2[d], beam_key(rv[a], a));
        }
        __syncthreads();

        // ---- 3a: per touched node m1, m2, c1 and what lies behind them; the node's own new value
        const int nt = min(s_ntouched, M);
        for (int base = 0; base < nt; base += BEAM_BLOCK) {
            const int j = base + tid;
            const bool valid = j < nt;
            bool made = false, is_wide = false;
            int q = 0, P1 = -1;
            if (valid) {
                q = min(max(touched[j], 0), Q - 1);
                const beam_u64 k1 = beam_load(&key1[q]), k2 = beam_load(&key2[q]);
                float v1 = -INFINITY, v2 = -INFINITY;
                int id1 = BEAM_NONE, id2 = BEAM_NONE, c1 = -1;
                if (k1) {
                    beam_clear(&key1[q]);
                    id1 = min(max(beam_key_id(k1), 0), A - 1);
                    v1 = rv[id1];
                    c1 = col_of(id1);
                }
                if (k2) {
                    beam_clear(&key2[q]);
                    id2 = min(max(beam_key_id(k2), 0), A - 1);
                    v2 = rv[id2];
                }
                const bool alive = ns[q] == tag_in;
                const float np = alive ? nv[q] : -INFINITY;                   // n_{t-1}[q]
                const int mine = alive ? npos[q] : -1;
                float M1 = np, M2 = np;
                int P2 = mine;
                P1 = mine;
                if (v1 > M1) { M1 = v1; P1 = rpos[id1]; }
                if (v2 > M2) { M2 = v2; P2 = rpos[id2]; }
                tm1[j] = M1; tm2[j] = M2; tc1[j] = c1; tp1[j] = P1; tp2[j] = P2;
                const float nn = lp0 + M1;
                if (nn > -INFINITY) {
                    nv[q] = nn;
                    ns[q] = tag_out;
                    lmax = fmaxf(lmax, nn);
                    made = true;
                }
                const int lo = min(max(p.out_ptr[q], 0), A), hi = min(max(p.out_ptr[q + 1], lo), A);
                is_wide = hi - lo > BEAM_WIDE;
            }
            const int ci = beam_append(&s_ncand, made);
            if (made && ci < QA) cand[ci] = make_int2(q, P1);
            const int wi = beam_append(&s_nwide, is_wide);
            if (is_wide && wi < M) wide[wi] = j;
        }
        __syncthreads();

        // ---- 3b: the arcs leaving the touched nodes
        auto make_arc = [&](bool has, int a, float M1, float M2, int c1, int P1, int P2) {
            bool made = false;
            int pred = -1;
            if (has) {
                const int k = col_of(a);
                const bool other = c1 != k;
                const float cnd = (other ? M1 : M2) + p.w[a];
                const bool alive = rs[a] == tag_in;
                float best = alive ? rv[a] : -INFINITY;
                pred = alive ? rpos[a] : -1;
                if (cnd > best) { best = cnd; pred = other ? P1 : P2; }
                const float v = row[1 + k] + best;
                if (v > -INFINITY) {
                    rv[a] = v;
                    rs[a] = tag_out;
                    lmax = fmaxf(lmax, v);
                    made = true;
                }
            }
            const int ci = beam_append(&s_ncand, made);
            if (made && ci < QA) cand[ci] = make_int2(Q + a, pred);
        };
        for (int base = 0; base < nt; base += BEAM_BLOCK) {
            const int j = base + tid;
            int lo = 0, deg = 0, c1 = -1, P1 = -1, P2 = -1;
            float M1 = -INFINITY, M2 = -INFINITY;
            if (j < nt) {
                const int q = min(max(touched[j], 0), Q - 1);
                lo = min(max(p.out_ptr[q], 0), A);
                deg = min(max(p.out_ptr[q + 1], lo), A) - lo;
                if (deg > BEAM_WIDE) deg = 0;                                 // a wave's, below
                if (deg) { M1 = tm1[j]; M2 = tm2[j]; c1 = tc1[j]; P1 = tp1[j]; P2 = tp2[j]; }
            }
            for (int e = 0; e < BEAM_WIDE; ++e) {
                const bool has = e < deg;
                if (__ballot(has) == 0) break;                                // the same for the whole wave
                make_arc(has, has ? min(max(p.out_arc[lo + e], 0), A - 1) : 0, M1, M2, c1, P1, P2);
            }
        }
        const int nw = min(s_nwide, M);
        for (int i = wave; i < nw; i += BEAM_WAVES) {
            const int j = min(max(wide[i], 0), nt - 1);
            const int q = min(max(touched[j], 0), Q - 1);
            const int lo = min(max(p.out_ptr[q], 0), A), deg = min(max(p.out_ptr[q + 1], lo), A) - lo;
            const float M1 = tm1[j], M2 = tm2[j];
            const int c1 = tc1[j], P1 = tp1[j], P2 = tp2[j];
            for (int e0 = 0; e0 < deg; e0 += 64) {
                const bool has = e0 + lane < deg;
                make_arc(has, has ? min(max(p.out_arc[lo + e0 + lane], 0), A - 1) : 0, M1, M2, c1, P1, P2);
            }
        }
        __syncthreads();
        if (tid == 0) { s_ntouched = 0; s_nwide = 0; }

        // ---- 4: the arcs of L_t whose src has no alive state: stay
        for (int base = 0; base < n; base += BEAM_BLOCK) {
            const int i = base + tid;
            bool made = false;
            int a = 0;
            if (i < n) {
                const int c = t ? Lin[i].x : 0;
                if (c >= Q) {
                    a = c - Q;
                    if (rs[a] == tag_in) {
                        const float v = row[1 + col_of(a)] + rv[a];
                        if (v > -INFINITY) {
                            rv[a] = v;
                            rs[a] = tag_out;
                            lmax = fmaxf(lmax, v);
                            made = true;
                        }
                    }
                }
            }
            const int ci = beam_append(&s_ncand, made);
            if (made && ci < QA) cand[ci] = make_int2(Q + a, i);
        }

        // ---- 5: best_t, thr_t
        lmax = wave_max(lmax);
        if (lane == 0) red_v[wave] = lmax;
        __syncthreads();
        float best = red_v[0];
#pragma unroll
        for (int i = 1; i < BEAM_WAVES; ++i) best = fmaxf(best, red_v[i]);
        const float thr = t < Tb - 1 ? best - p.beam : -INFINITY;

        // ---- 6: prune; the survivors are L_{t+1}
        const int nc = min(s_ncand, QA);
        for (int base = 0; base < nc; base += BEAM_BLOCK) {
            const int i = base + tid;
            const bool valid = i < nc;
            bool keep = false;
            int2 e = make_int2(0, -1);
            if (valid) {
                e = cand[i];
                const float v = e.x < Q ? nv[e.x] : rv[e.x - Q];
                keep = !(v < thr);
                if (!keep) { if (e.x < Q) ns[e.x] = 0; else rs[e.x - Q] = 0; }
            }
            const int si = beam_append(&s_nsurv, keep);
            if (keep && si < M) {
                Lout[si] = e;
                if (e.x < Q) npos[e.x] = si; else rpos[e.x - Q] = si;
            }
        }
        __syncthreads();
        const int cnt = s_nsurv;
        peak = max(peak, cnt);
        if (cnt > p.max_active) { status = OE_CTC_GRAPH_BEAM_OVERFLOW; peak = cnt; break; }
        n = cnt;
        if (cnt == 0) break;
        done = t + 1;
    }

    // ---- the end: the best of value + final over the last list, the lowest state id on ties (nodes, then arcs)
    float bv = -INFINITY;
    int bi = BEAM_NONE, bp = -1;
    if (Tb > 0 && done == Tb) {
        const int2* L = rec + (size_t)(Tb - 1) * Mp;
        for (int i = tid; i < n; i += BEAM_BLOCK) {
            const int c = L[i].x;
            const float v = c < Q ? nv[c] + p.fin[c] : rv[c - Q] + p.fin[dst_of(c - Q)];
            if (graph_better(v, c, bv, bi)) { bv = v; bi = c; bp = i; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v = __shfl_xor(bv, o, 64);
        const int i = __shfl_xor(bi, o, 64), q = __shfl_xor(bp, o, 64);
        if (graph_better(v, i, bv, bi)) { bv = v; bi = i; bp = q; }
    }
    __syncthreads();                                                          // red_v was read in the last frame
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_p[wave] = bp; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < BEAM_WAVES; ++i)
            if (graph_better(red_v[i], red_i[i], bv, bi)) { bv = red_v[i]; bi = red_i[i]; bp = red_p[i]; }
        const bool ok = bv > -INFINITY;
        end_state = ok ? bi : -1;
        p.score[b] = ok ? bv : -INFINITY;
        p.status[b] = status == OE_CTC_GRAPH_BEAM_OVERFLOW ? status : ok ? OE_CTC_GRAPH_BEAM_OK : OE_CTC_GRAPH_BEAM_INFEASIBLE;
        p.peak[b] = peak;
        // ---- back-trace along the positions: entry pos of L_{t+1} is the state of frame t
        if (ok) {
            int pos = bp;
            for (int t = Tb - 1; t >= 0; --t) {
                const int2 e = rec[(size_t)t * Mp + min(max(pos, 0), M - 1)];
                if (e.x >= Q) {
                    const int a = min(e.x - Q, A - 1);
                    frames[t] = p.label[a];
                    arcs[t] = a;
                    if (path_logp) path_logp[t] = cw[(long)t * rw + 1 + col_of(a)];
                } else {
                    frames[t] = 0;
                    arcs[t] = -1;
                    if (path_logp) path_logp[t] = cw[(long)t * rw];
                }
                pos = e.y;
            }
        }
    }
    __syncthreads();
    const bool ok = end_state >= 0;
    for (int t = (ok ? Tb : 0) + tid; t < T; t += BEAM_BLOCK) {
        frames[t] = -1;
        arcs[t] = -1;
        if (path_logp) path_logp[t] = 0.f;
    }

    // ---- traversals (ctc_graph.hip): a start at t iff arcs[t] >= 0 and (t == 0 or arcs[t-1] != arcs[t]); slots in frame order
    int* ta = p.trav_arc + (long)b * max_trav;
    int* ts = p.trav_start + (long)b * max_trav;
    int* te = p.trav_end + (long)b * max_trav;
    float* tl = p.trav_logp ? p.trav_logp + (long)b * max_trav : nullptr;
    int count = 0;
    if (ok) {
        for (int c0 = 0; c0 < Tb; c0 += BEAM_BLOCK) {
            const int t = c0 + tid;
            const int a = t < Tb ? arcs[t] : -1;
            const bool start = a >= 0 && (t == 0 || arcs[t - 1] != a);
            const beam_u64 m = __ballot(start);
            if (lane == 0) red_i[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
            for (int i = 0; i < BEAM_WAVES; ++i) {
                const int k = red_i[i];
                if (i < wave) before += k;
                total += k;
            }
            const int slot = count + before + __popcll(m & ((1ull << lane) - 1ull));
            if (start && slot < max_trav) {
                const int k = col_of(a);
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
    for (int i = min(count, max_trav) + tid; i < max_trav; i += BEAM_BLOCK) {
        ta[i] = -1; ts[i] = -1; te[i] = -1;
        if (tl) tl[i] = 0.f;
    }
    if (tid == 0) p.n_trav[b] = count;
}

// ---------------------------------------------------------------- host -------
static bool beam_shape_ok(long B, long T, long U, long Q, long A, long max_active) {
    return B > 0 && T > 0 && T <= BEAM_MAX_T && U > 0 && Q >= 1 && Q <= BEAM_MAX_Q && A >= 1 && A <= BEAM_MAX_A && max_active >= 1;
}
static size_t beam_rows_bytes(long B, long T, long U) { return ((size_t)B * (size_t)T * ((size_t)U + 1) * 4 + 15) & ~(size_t)15; }
static long beam_capacity(long Q, long A, long max_active) { return max_active < Q + A ? max_active : Q + A; }

extern "C" size_t oe_ctc_graph_beam_workspace_bytes(int B, int T, int U, int Q, int A, int max_active) {
    if (!beam_shape_ok(B, T, U, Q, A, max_active)) return 0;
    return beam_rows_bytes(B, T, U) + (size_t)B * beam_layout(T, Q, A, beam_capacity(Q, A, max_active)).bytes;
}

extern "C" int oe_ctc_graph_beam(const oe_ctc_graph_beam_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph_beam: null args");
    const oe_ctc_graph_beam_args& a = *args;
    if (int rc = graph_check("oe_ctc_graph_beam", a.graph, a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.workspace, &a.max_trav)) return rc;
    const oe_beam_graph& g = *a.graph;
    OE_REQUIRE(a.score && a.frames && a.arcs && a.n_trav && a.trav_arc && a.trav_start && a.trav_end && a.status && a.peak,
               "oe_ctc_graph_beam: null output (score, frames, arcs, n_trav, trav_arc, trav_start, trav_end, status, peak)");
    OE_REQUIRE(g.Q >= 1 && g.Q <= BEAM_MAX_Q, "oe_ctc_graph_beam: Q=%d nodes outside 1 .. %d", g.Q, BEAM_MAX_Q);
    OE_REQUIRE(g.A >= 1 && g.A <= BEAM_MAX_A, "oe_ctc_graph_beam: A=%d arcs outside 1 .. %d", g.A, BEAM_MAX_A);
    OE_REQUIRE(g.in_ptr && g.src && g.dst && g.label && g.col && g.w && g.final && g.cols && g.out_ptr && g.out_arc,
               "oe_ctc_graph_beam: null table in graph (in_ptr, src, dst, label, col, w, final, cols, out_ptr, out_arc)");
    OE_REQUIRE(a.max_active >= 1, "oe_ctc_graph_beam: max_active=%d < 1", a.max_active);
    OE_REQUIRE(a.beam >= 0.f, "oe_ctc_graph_beam: beam=%g is not >= 0 (+inf: no pruning)", (double)a.beam);
    hipStream_t st = (hipStream_t)stream;
    float* cw = reinterpret_cast<float*>(a.workspace);
    if (int rc = oe_lp_rows("oe_ctc_graph_beam", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, g.cols, g.U, a.normalized, cw, nullptr, st))
        return rc;
    BeamParams p;
    p.cw = cw;
    p.ws = reinterpret_cast<char*>(a.workspace) + beam_rows_bytes(a.B, a.T, g.U);
    p.M = (int)beam_capacity(g.Q, g.A, a.max_active);
    p.l = beam_layout(a.T, g.Q, g.A, p.M);
    p.T = a.T; p.U = g.U; p.Q = g.Q; p.A = g.A; p.max_active = a.max_active; p.max_trav = a.max_trav; p.beam = a.beam;
    p.hlens = a.hlens; p.dst = g.dst; p.label = g.label; p.col = g.col; p.w = g.w; p.fin = g.final;
    p.out_ptr = g.out_ptr; p.out_arc = g.out_arc;
    p.score = a.score; p.frames = a.frames; p.arcs = a.arcs; p.path_logp = a.path_logp;
    p.n_trav = a.n_trav; p.trav_arc = a.trav_arc; p.trav_start = a.trav_start; p.trav_end = a.trav_end; p.trav_logp = a.trav_logp;
    p.status = a.status; p.peak = a.peak;
    hipLaunchKernelGGL(beam_kernel, dim3((unsigned)a.B), dim3(BEAM_BLOCK), 0, st, p);
    OE_LAUNCH_CHECK("ctc_graph_beam");
    return 0;
}
