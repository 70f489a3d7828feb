// N-best grammar-constrained CTC decoding: the K best distinct paths of the CTC posteriors through a token graph, each scored by
// its best alignment.  The semantics every layer refers to are in include/openeat_hip.h (oe_ctc_graph_nbest); the graph, the
// states, lp, the clamping and the float32 arithmetic are oe_ctc_graph's (ctc_graph.hip), with an ordered list of at most K
// tokens (value, history) per state in place of one value.
//
// A token is 16 bytes: its value, the id of the record of its last "enter an arc" event, and the 64-bit hash of its history.
// Two launches:
//   launch 1  lp_rows_kernel (lp_rows.hip): the blank and the U label columns of every frame as lp, a compact row of U + 1 floats.
//   launch 2  graph_nbest_kernel<KC, BLOCK>: ONE WORKGROUP PER UTTERANCE, KC in {1, 2, 4, 8} the compiled list capacity
//             (K <= KC; 1024 threads for KC <= 2, 512 for the longer lists, which then have 256 registers a thread and keep a
//             list in them).  The token lists do not fit the LDS at the limits; they live in the workspace (L2), the arc
//             lists and the node lists double-buffered.  A selection is a stream through a sorted register list (NbList):
//             candidates arrive in candidate order, a history already held keeps its better value, a new one goes behind
//             equal values, and a sorted source list is left at its first token that does not enter.  A frame is three phases
//             with a barrier behind each:
//             A1 per node q: G[q] = select_K of (the node's tokens, then the tokens of every incoming arc): n_t[q] before lp[t,0]
//                is added.  Nodes of in-degree <= 32 take a thread each; the others a wave each: a lane streams every 64th arc
//                into a list of its own, which then holds whatever of its share can be among the K best, and K rounds of
//                "the best untaken head over the lanes", by a wave reduction over (value, candidate order), finish.  Then the
//                node's "affected" labels: the labels of the last arcs of G's histories, at most K.  A token of an arc of
//                label c holds a history that ends in c, so for any other label no token of that label sits in the sorted
//                prefix that produced G, and the filtered selection "every incoming arc of another label" IS G.
//             A2 per (node, affected label c): the filtered selection over the incoming arcs whose label is not c, the same
//                routine: for a light node by its own thread right behind A1, for a wide node a wave per label.
//             B  per arc a: E = the list of src[a] for label[a] (an A2 list if the label is affected, else G); the stay tokens,
//                then E + w[a] with the arc appended to the history, through one list (stay first: they win ties); lp
//                added; an entered token gets the record (t, a, slot) holding its parent record.
//             A frame costs O((Q + A) * K^2) list steps where the affected labels are few (tries, chains) and up to K times
//             that at a node all of whose K best histories end in different labels.
//             Then: the end rule by K workgroup rounds of "the best untaken head over the final states", and one thread per
//             hypothesis walks its record chain (twice: the length, then the arcs).
// No workgroup waits for another, no float atomics, no allocation, no host read: capturable.
#include <stdlib.h>
#include "ctc_graph_common.h"
#include "../../include/openeat_hip.h"

#define NB_BLOCK 1024
#define NB_MAX_T GRAPH_MAX_T
#define NB_MAX_A OE_CTC_GRAPH_MAX_ARCS
#define NB_MAX_Q OE_CTC_GRAPH_MAX_NODES
#define NB_MAX_K OE_CTC_GRAPH_NBEST_MAX
#define NB_HEAVY 32                               // a node of more incoming arcs than this takes a wave, not a thread
#define NB_MAX_HEAVY (NB_MAX_A / (NB_HEAVY + 1) + 1)
#define NB_NONE 0x7fffffff

static_assert(NB_MAX_K == 8, "oe_ctc_graph_nbest: the kernel is instantiated for list capacities 1, 2, 4, 8");

struct __attribute__((aligned(16))) NbTok { float v; int rec; unsigned long long h; };
static_assert(sizeof(NbTok) == 16, "oe_ctc_graph_nbest: a token is 16 bytes");

// the history hash: the splitmix64 finaliser over (h, id + 1); the empty history is 0
__device__ __forceinline__ unsigned long long nb_mix(unsigned long long h, int id) {
    unsigned long long z = h + 0x9E3779B97F4A7C15ull * (unsigned long long)(id + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------- launch 2 ----
struct NbParams {
    const float* cw;
    NbTok* rl; NbTok* nl; NbTok* alt; int* alt_col; int* recs;                // per utterance: 2*A*K, 2*Q*K, Q*K*K tokens; Q*K, T*A*K ints
    int T, U, Q, A, K, max_len, tokens_mode;
    const int* hlens; const int* in_ptr; const int* src; const int* dst; const int* label; const int* col;
    const float* w; const float* fin;
    int* n_hyp; float* hyp_score; int* hyp_len; int* hyp_arcs; int* hyp_tokens;
};

// A sorted list of at most KC tokens with distinct histories, in registers (every index is static).  aux: the candidate's order
// key where lists of several lanes are merged, "entered" in phase B.
template <int KC>
struct NbList {
    float v[KC]; unsigned long long h[KC]; int rec[KC]; int aux[KC];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < KC; ++i) { v[i] = -INFINITY; h[i] = 0; rec[i] = -1; aux[i] = NB_NONE; }
    }
    // select_K as a stream: candidates arrive in candidate order.  A history already held keeps the better value (the earlier
    // one on ties); a new one goes behind the values equal to its own; what falls off the end has KC better histories before it.
    // Returns false if the candidate was at or below a full list's last value (so is everything behind it in a sorted list).
    __device__ __forceinline__ bool push(float cv, unsigned long long ch, int crec, int caux) {
        if (!(cv > v[KC - 1])) return false;
        int dp = KC;
#pragma unroll
        for (int i = 0; i < KC; ++i)
            if (h[i] == ch && v[i] > -INFINITY) dp = i;
        if (dp < KC) {
            bool better = false;
#pragma unroll
            for (int i = 0; i < KC; ++i) better |= i == dp && cv > v[i];
            if (!better) return true;
#pragma unroll
            for (int i = 0; i < KC - 1; ++i)
                if (i >= dp) { v[i] = v[i + 1]; h[i] = h[i + 1]; rec[i] = rec[i + 1]; aux[i] = aux[i + 1]; }
            v[KC - 1] = -INFINITY; h[KC - 1] = 0; rec[KC - 1] = -1; aux[KC - 1] = NB_NONE;
        }
        int pos = 0;
#pragma unroll
        for (int i = 0; i < KC; ++i) pos += v[i] >= cv;
#pragma unroll
        for (int i = KC - 1; i > 0; --i)
            if (i > pos) { v[i] = v[i - 1]; h[i] = h[i - 1]; rec[i] = rec[i - 1]; aux[i] = aux[i - 1]; }
#pragma unroll
        for (int i = 0; i < KC; ++i)
            if (i == pos) { v[i] = cv; h[i] = ch; rec[i] = crec; aux[i] = caux; }
        return true;
    }
};

// select_K over the candidates of a node in their order - the tokens of the node's previous list (lp0_prev added), then those
// of the incoming arcs lo .. hi-1 whose column is not fc (fc < 0: no filter) - into out[0 .. K), unused slots unreachable.
// The lists hold KC >= K histories; the first K of the KC best are the K best.  A thread streams every candidate through one
// list.  WAVE: a lane streams every 64th arc (lane 0 the node's tokens first) into a list of its own, which then holds every
// token of its share that can be among the best; K rounds of "the best untaken head over the lanes" (value, then candidate
// order) finish, every lane ending with the same result; lane 0 writes.  recs_out: the records selected (NB_NONE behind).
template <int KC, bool WAVE>
__device__ __forceinline__ int nb_select(const NbTok* nprev, float lp0_prev, const NbTok* rl, const int* colp, int U, int K, int lo,
                                         int hi, int fc, int lane, NbTok* out, int (&recs_out)[KC]) {
    NbList<KC> L;
    L.clear();
    if (!WAVE || lane == 0) {
        NbTok tk[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < K) tk[j] = nprev[j];
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < K && tk[j].v > -INFINITY) {
                const float v = lp0_prev + tk[j].v;
                if (v > -INFINITY) L.push(v, tk[j].h, tk[j].rec, j);
            }
    }
    for (int a = lo + (WAVE ? lane : 0); a < hi; a += WAVE ? 64 : 1) {
        if (fc >= 0 && min(max(colp[a], 0), U - 1) == fc) continue;
        const NbTok* l = rl + (long)a * K;
        NbTok tk[KC];
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < K) tk[j] = l[j];
        bool live = true;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < K && live) live = tk[j].v > -INFINITY && L.push(tk[j].v, tk[j].h, tk[j].rec, (a - lo + 1) * K + j);
    }
    int n = 0;
    if (!WAVE) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            recs_out[k] = NB_NONE;
            if (k < K) {
                NbTok o; o.v = L.v[k]; o.rec = L.rec[k]; o.h = L.h[k];
                out[k] = o;
                if (L.v[k] > -INFINITY) { recs_out[k] = L.rec[k]; n = k + 1; }
            }
        }
        return n;
    }
    unsigned long long th[KC];
    bool done = false;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        recs_out[k] = NB_NONE;
        th[k] = 0;
        if (k < K && !done) {
            float bv = -INFINITY;                                            // this lane's best untaken token: the first one, the list is sorted
            int bo = NB_NONE, brec = -1;
            unsigned long long bh = 0;
#pragma unroll
            for (int j = KC - 1; j >= 0; --j) {
                bool dup = !(L.v[j] > -INFINITY);
#pragma unroll
                for (int i = 0; i < k; ++i) dup |= th[i] == L.h[j];
                if (!dup) { bv = L.v[j]; bo = L.aux[j]; brec = L.rec[j]; bh = L.h[j]; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float v = __shfl_xor(bv, o, 64);
                const int i = __shfl_xor(bo, o, 64);
                const int r = __shfl_xor(brec, o, 64);
                const unsigned long long hh = __shfl_xor(bh, o, 64);
                if (graph_better(v, i, bv, bo)) { bv = v; bo = i; brec = r; bh = hh; }
            }
            if (!(bv > -INFINITY)) done = true;
            else {
                th[k] = bh;
                recs_out[k] = brec;
                if (lane == 0) { NbTok o; o.v = bv; o.rec = brec; o.h = bh; out[k] = o; }
                n = k + 1;
            }
        }
    }
    if (lane == 0)
        for (int k = n; k < K; ++k) { NbTok o; o.v = -INFINITY; o.rec = -1; o.h = 0; out[k] = o; }
    return n;
}

template <int KC, int BLOCK>
__global__ __launch_bounds__(BLOCK) void graph_nbest_kernel(const NbParams p) {
    __shared__ unsigned short heavy[NB_MAX_HEAVY];
    __shared__ int n_heavy;
    __shared__ float red_v[BLOCK / 64];
    __shared__ int red_i[BLOCK / 64];
    __shared__ int hyp_rec[NB_MAX_K];
    __shared__ int hyp_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int T = p.T, U = p.U, Q = p.Q, A = p.A, K = p.K, max_len = p.max_len;
    const int Tb = max(min(p.hlens[b], T), 0);
    const long rw = U + 1;
    const float* cw = p.cw + (long)b * T * rw;
    NbTok* rl = p.rl + (long)b * 2 * A * K;
    NbTok* nl = p.nl + (long)b * 2 * Q * K;
    NbTok* alt = p.alt + (long)b * Q * K * K;
    int* alt_col = p.alt_col + (long)b * Q * K;
    int* recs = p.recs + (long)b * T * A * K;

    // ---- before frame 0: n[0] holds one token (0, the empty history), every other list is empty; the list of wide nodes
    for (long i = tid; i < (long)A * K; i += BLOCK) { NbTok o; o.v = -INFINITY; o.rec = -1; o.h = 0; rl[i] = o; }
    for (long i = tid; i < (long)Q * K; i += BLOCK) { NbTok o; o.v = i == 0 ? 0.f : -INFINITY; o.rec = -1; o.h = 0; nl[i] = o; }
    if (tid == 0) n_heavy = 0;
    __syncthreads();
    for (int q = tid; q < Q; q += BLOCK) {
        const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
        if (hi - lo > NB_HEAVY) {
            const int i = atomicAdd(&n_heavy, 1);                            // the order of the list does not reach the results
            if (i < NB_MAX_HEAVY) heavy[i] = (unsigned short)q;
        }
    }
    __syncthreads();
    const int nh = min(n_heavy, NB_MAX_HEAVY);

    float lp0_prev = 0.f;
    int cur = 0;                                                             // the buffer that holds the lists of frame t-1
    for (int t = 0; t < Tb; ++t) {
        const float* row = cw + (long)t * rw;
        const NbTok* rprev = rl + (long)cur * A * K;
        NbTok* rnext = rl + (long)(cur ^ 1) * A * K;
        const NbTok* nprev = nl + (long)cur * Q * K;
        NbTok* nnext = nl + (long)(cur ^ 1) * Q * K;

        // ---- phase A1: per node, G and the affected labels
        auto labels_of = [&](int q, const int (&rc)[KC]) {
            int* ac = alt_col + (long)q * K;
            int nc = 0;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                if (k < K && rc[k] != NB_NONE && rc[k] >= 0) {
                    const int a = (rc[k] / K) % A;
                    const int c = min(max(p.col[a], 0), U - 1);
                    bool seen = false;
                    for (int i = 0; i < nc; ++i) seen |= ac[i] == c;
                    if (!seen) ac[nc++] = c;
                }
            }
            for (; nc < K; ++nc) ac[nc] = -1;
        };
        for (int q = tid; q < Q; q += BLOCK) {
            const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
            if (hi - lo > NB_HEAVY) continue;
            int rc[KC];
            nb_select<KC, false>(nprev + (long)q * K, lp0_prev, rprev, p.col, U, K, lo, hi, -1, 0, nnext + (long)q * K, rc);
            labels_of(q, rc);
            for (int j = 0; j < K; ++j) {                                    // phase A2 of a light node, by the same thread
                const int fc = alt_col[(long)q * K + j];
                if (fc < 0) break;
                nb_select<KC, false>(nprev + (long)q * K, lp0_prev, rprev, p.col, U, K, lo, hi, fc, 0, alt + ((long)q * K + j) * K, rc);
            }
        }
        for (int i = wave; i < nh; i += (BLOCK / 64)) {
            const int q = heavy[i];
            const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
            int rc[KC];
            nb_select<KC, true>(nprev + (long)q * K, lp0_prev, rprev, p.col, U, K, lo, hi, -1, lane, nnext + (long)q * K, rc);
            if (lane == 0) labels_of(q, rc);
        }
        __syncthreads();

        // ---- phase A2: per (wide node, affected label), the selection without the arcs of that label
        for (int i = wave; i < nh * K; i += (BLOCK / 64)) {
            const int q = heavy[i / K];
            const long item = (long)q * K + i % K;
            const int fc = alt_col[item];
            if (fc < 0) continue;
            const int lo = min(max(p.in_ptr[q], 0), A), hi = min(max(p.in_ptr[q + 1], lo), A);
            int rc[KC];
            nb_select<KC, true>(nprev + (long)q * K, lp0_prev, rprev, p.col, U, K, lo, hi, fc, lane, alt + item * K, rc);
        }
        if (nh > 0) __syncthreads();

        // ---- phase B: per arc, the stay tokens merged with E + w
        for (int a = tid; a < A; a += BLOCK) {
            const int s = min(max(p.src[a], 0), Q - 1);
            const int c = min(max(p.col[a], 0), U - 1);
            const float w = p.w[a];
            const float lp = row[1 + c];
            const int id = p.tokens_mode ? c : a;
            const NbTok* E = nnext + (long)s * K;
            for (int j = 0; j < K; ++j) {
                const int ac = alt_col[(long)s * K + j];
                if (ac < 0) break;
                if (ac == c) { E = alt + ((long)s * K + j) * K; break; }
            }
            const NbTok* S = rprev + (long)a * K;
            NbTok* O = rnext + (long)a * K;
            NbList<KC> L;                                                    // rec: a stay token's record, an entered token's parent; aux: entered
            L.clear();
            NbTok et[KC];
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < K) et[j] = S[j];
#pragma unroll
            for (int j = 0; j < KC; ++j)                                     // the stay tokens come first: they win ties
                if (j < K && et[j].v > -INFINITY) L.push(et[j].v, et[j].h, et[j].rec, 0);
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < K) et[j] = E[j];
            bool live = true;
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < K && live) live = et[j].v > -INFINITY && L.push(et[j].v + w, nb_mix(et[j].h, id), et[j].rec, 1);
#pragma unroll
            for (int n = 0; n < KC; ++n) {
                if (n < K) {
                    NbTok o; o.v = -INFINITY; o.rec = -1; o.h = 0;
                    if (L.v[n] > -INFINITY) {
                        int rec = L.rec[n];
                        if (L.aux[n] == 1) {
                            rec = (t * A + a) * K + n;
                            recs[rec] = L.rec[n];
                        }
                        o.v = lp + L.v[n]; o.rec = rec; o.h = L.h[n];
                    }
                    O[n] = o;
                }
            }
        }
        __syncthreads();
        lp0_prev = row[0];
        cur ^= 1;
    }

    // ---- the end: select_K over the final states, nodes by ascending q, then arcs by ascending id
    float* hs = p.hyp_score + (long)b * K;
    int* hl = p.hyp_len + (long)b * K;
    int* ha = p.hyp_arcs + (long)b * K * max_len;
    int* ht = p.hyp_tokens + (long)b * K * max_len;
    for (long i = tid; i < (long)K * max_len; i += BLOCK) { ha[i] = -1; ht[i] = -1; }
    if (tid < K) { hs[tid] = -INFINITY; hl[tid] = -1; }
    if (tid == 0) hyp_count = 0;
    __syncthreads();
    if (Tb > 0) {
        const NbTok* rend = rl + (long)cur * A * K;
        const NbTok* nend = nl + (long)cur * Q * K;
        unsigned long long th[KC];
        bool done = false;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            th[k] = 0;
            if (k < K && !done) {
                float bv = -INFINITY;
                int bo = NB_NONE;
                for (int i = tid; i < Q + A; i += BLOCK) {
                    const bool node = i < Q;
                    const float f = p.fin[node ? i : min(max(p.dst[i - Q], 0), Q - 1)];
                    if (!(f > -INFINITY)) continue;
                    const NbTok* l = node ? nend + (long)i * K : rend + (long)(i - Q) * K;
                    for (int j = 0; j < K; ++j) {
                        const NbTok tk = l[j];
                        if (!(tk.v > -INFINITY)) break;
                        bool dup = false;
#pragma unroll
                        for (int x = 0; x < k; ++x) dup |= th[x] == tk.h;
                        if (dup) continue;
                        const float v = (node ? lp0_prev + tk.v : tk.v) + f;
                        if (v > bv) { bv = v; bo = i * K + j; }
                        break;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float v = __shfl_xor(bv, o, 64);
                    const int i = __shfl_xor(bo, o, 64);
                    if (graph_better(v, i, bv, bo)) { bv = v; bo = i; }
                }
                if (lane == 0) { red_v[wave] = bv; red_i[wave] = bo; }
                __syncthreads();
                bv = red_v[0]; bo = red_i[0];
                for (int i = 1; i < (BLOCK / 64); ++i)
                    if (graph_better(red_v[i], red_i[i], bv, bo)) { bv = red_v[i]; bo = red_i[i]; }
                __syncthreads();
                if (!(bv > -INFINITY)) done = true;
                else {
                    const int st = bo / K;
                    const NbTok tk = st < Q ? nend[(long)st * K + bo % K] : rend[(long)(st - Q) * K + bo % K];
                    th[k] = tk.h;
                    if (tid == 0) { hs[k] = bv; hyp_rec[k] = tk.rec; hyp_count = k + 1; }
                }
            }
        }
    }
    __syncthreads();
    const int nhyp = hyp_count;
    if (tid == 0) p.n_hyp[b] = nhyp;
    // ---- the paths: one thread per hypothesis walks its record chain, the length first
    if (tid < nhyp) {
        int len = 0;
        for (int r = hyp_rec[tid]; r >= 0; r = recs[r]) ++len;
        hl[tid] = len;
        int pos = len - 1;
        for (int r = hyp_rec[tid]; r >= 0; r = recs[r], --pos) {
            if (pos < max_len) {
                const int a = (r / K) % A;
                ha[(long)tid * max_len + pos] = a;
                ht[(long)tid * max_len + pos] = p.label[a];
            }
        }
    }
}

// ---------------------------------------------------------------- host -------
static bool nbest_shape_ok(long B, long T, long U, long Q, long A, long K) {
    return B > 0 && T > 0 && T <= NB_MAX_T && U > 0 && Q >= 1 && Q <= NB_MAX_Q && A >= 1 && A <= NB_MAX_A && K >= 1 && K <= NB_MAX_K &&
           T * A * K < (1l << 31);
}
// per utterance: the token lists (16 bytes a token), then the affected labels, the record table and the lp rows (4 bytes each)
static size_t nbest_tokens(size_t Q, size_t A, size_t K) { return K * (2 * A + 2 * Q + Q * K); }
static size_t nbest_words(size_t T, size_t U, size_t Q, size_t A, size_t K) { return Q * K + T * A * K + T * (U + 1); }

extern "C" size_t oe_ctc_graph_nbest_workspace_bytes(int B, int T, int U, int Q, int A, int nbest) {
    if (!nbest_shape_ok(B, T, U, Q, A, nbest)) return 0;
    const size_t words = (size_t)B * nbest_words(T, U, Q, A, nbest);
    return (size_t)B * nbest_tokens(Q, A, nbest) * 16 + (words + 3) / 4 * 16;
}

extern "C" int oe_ctc_graph_nbest(const oe_ctc_graph_nbest_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_graph_nbest: null args");
    const oe_ctc_graph_nbest_args& a = *args;
    if (int rc = graph_check("oe_ctc_graph_nbest", a.graph, a.logits, a.ldv, a.B, a.T, a.V, a.hlens, a.workspace, nullptr)) return rc;
    const oe_decoding_graph& g = *a.graph;
    OE_REQUIRE(a.n_hyp && a.hyp_score && a.hyp_len && a.hyp_arcs && a.hyp_tokens,
               "oe_ctc_graph_nbest: null output (n_hyp, hyp_score, hyp_len, hyp_arcs, hyp_tokens)");
    OE_REQUIRE(g.Q >= 1 && g.Q <= NB_MAX_Q, "oe_ctc_graph_nbest: Q=%d nodes outside 1 .. %d", g.Q, NB_MAX_Q);
    OE_REQUIRE(g.A >= 1 && g.A <= NB_MAX_A, "oe_ctc_graph_nbest: A=%d arcs outside 1 .. %d", g.A, NB_MAX_A);
    OE_REQUIRE(g.in_ptr && g.src && g.dst && g.label && g.col && g.w && g.final && g.cols,
               "oe_ctc_graph_nbest: null table in graph (in_ptr, src, dst, label, col, w, final, cols)");
    OE_REQUIRE(a.nbest >= 1 && a.nbest <= NB_MAX_K, "oe_ctc_graph_nbest: nbest=%d outside 1 .. %d", a.nbest, NB_MAX_K);
    OE_REQUIRE(a.max_len >= 1, "oe_ctc_graph_nbest: max_len=%d < 1", a.max_len);
    OE_REQUIRE(a.distinct == OE_CTC_GRAPH_NBEST_ARCS || a.distinct == OE_CTC_GRAPH_NBEST_TOKENS,
               "oe_ctc_graph_nbest: distinct=%d is neither OE_CTC_GRAPH_NBEST_ARCS (0) nor OE_CTC_GRAPH_NBEST_TOKENS (1)", a.distinct);
    OE_REQUIRE((long)a.T * g.A * a.nbest < (1l << 31), "oe_ctc_graph_nbest: T*A*nbest = %ld records, the limit is 2^31 - 1",
               (long)a.T * g.A * a.nbest);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = (size_t)a.B, T = (size_t)a.T, Q = (size_t)g.Q, A = (size_t)g.A, K = (size_t)a.nbest;
    NbParams p;
    p.rl = reinterpret_cast<NbTok*>(a.workspace);
    p.nl = p.rl + B * 2 * A * K;
    p.alt = p.nl + B * 2 * Q * K;
    p.alt_col = reinterpret_cast<int*>(p.alt + B * Q * K * K);
    p.recs = p.alt_col + B * Q * K;
    float* cw = reinterpret_cast<float*>(p.recs + B * T * A * K);
    p.cw = cw;
    if (int rc = oe_lp_rows("oe_ctc_graph_nbest", a.logits, a.ldv, a.B, a.T, a.V, a.hlens, g.cols, g.U, a.normalized, cw, nullptr, st))
        return rc;
    p.T = a.T; p.U = g.U; p.Q = g.Q; p.A = g.A; p.K = a.nbest; p.max_len = a.max_len; p.tokens_mode = a.distinct == OE_CTC_GRAPH_NBEST_TOKENS;
    p.hlens = a.hlens; p.in_ptr = g.in_ptr; p.src = g.src; p.dst = g.dst; p.label = g.label; p.col = g.col; p.w = g.w; p.fin = g.final;
    p.n_hyp = a.n_hyp; p.hyp_score = a.hyp_score; p.hyp_len = a.hyp_len; p.hyp_arcs = a.hyp_arcs; p.hyp_tokens = a.hyp_tokens;
    const dim3 grid((unsigned)a.B);                                         // the longer lists take 512 threads: 256 registers each
    if (a.nbest == 1) hipLaunchKernelGGL((graph_nbest_kernel<1, NB_BLOCK>), grid, dim3(NB_BLOCK), 0, st, p);
    else if (a.nbest == 2) hipLaunchKernelGGL((graph_nbest_kernel<2, NB_BLOCK>), grid, dim3(NB_BLOCK), 0, st, p);
    else if (a.nbest <= 4) hipLaunchKernelGGL((graph_nbest_kernel<4, NB_BLOCK / 2>), grid, dim3(NB_BLOCK / 2), 0, st, p);
    else hipLaunchKernelGGL((graph_nbest_kernel<8, NB_BLOCK / 2>), grid, dim3(NB_BLOCK / 2), 0, st, p);
    OE_LAUNCH_CHECK("ctc_graph_nbest");
    return 0;
}
