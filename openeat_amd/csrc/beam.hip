// CTC prefix beam search on the device, one wavefront per utterance, plain, with n-gram LM shallow fusion and with hotword
// biasing: one kernel source, template <bool LM, bool CTX, bool CHUNK>, one entry point for the search over a whole utterance
// (oe_ctc_prefix_beam: its oe_prefix_beam_args name the n-gram model and the context graph, or neither; semantics in
// include/openeat_hip.h) and one for the resumable search, which takes the frames chunk by chunk and carries a device state
// between them (oe_ctc_prefix_beam_chunk, CHUNK = true: the same frame loop, entered from a saved state and left into one; what
// it adds is described above the kernel and sits under `if constexpr (CHUNK)`).
// (the reference's openeat/models/asr_model.py:359-396: the per-frame Python dict loop).
//
// Same arithmetic and the same ordering as the reference and as the host implementation (beam_host.cpp, which stays as
// the checker): python floats = doubles, log_add = max + log(sum exp(. - max)) accumulated in the order the reference
// visits (token j of the frame's top-k, then hypothesis h), pruning = stable sort by log_add(pb, pnb) descending, i.e.
// ties keep the dict's insertion order.
//
// What makes it parallel.  In one frame every entry of next_hyps receives a bounded, known set of updates:
//   * the entry of a current prefix n ("stay"): at most ONE update of pb (the blank, if it is in the top-k) and at most
//     TWO of pnb - the repeated last token without extension (from n itself) and the extension of n's parent m by n's
//     last token (from m, only if m is also in the beam) - both at the same j, so their order is the order of n and m in
//     the beam;
//   * the entry of a new prefix n + [s]: exactly one update.
// So the wave evaluates all beam x beam (token, hypothesis) pairs at once (lane = pair), routes the few extension
// candidates that land on an existing prefix to that prefix's lane through LDS, applies each entry's updates in the
// reference's order, stamps every entry with the sequence number of its first touch (2 (j |beam| + h) + {0: the
// hypothesis' own entry, 1: its extension}), and picks the best `beam` entries by (score descending, stamp ascending) in
// `beam` rounds of a wave-wide arg-max.  Prefixes are identified by (64-bit polynomial hash of the token sequence,
// length) instead of the host version's trie - equal prefixes always meet, distinct ones collide with probability
// ~2^-64 per pair - and their tokens are recovered at the end by walking per-frame back-pointers (slot of the parent,
// token appended) kept in a workspace.
// Differences from the host version: exp / log are the device's double-precision routines (<= 1 ulp, not glibc's), so a
// score can differ in its last bits.
//
// The fusion (LM = true) is this recursion with ONE change - the key that orders next_hyps before the cut to `beam` is
//   total(p) = log_add(pb, pnb) + lm_weight * LM(p) + length_bonus * len(p)
// instead of log_add(pb, pnb) - plus, at the end of the utterance, the optional </s> term and a stable re-sort of the
// survivors by total.  Everything it adds sits under `if constexpr (LM)`; the pb / pnb arithmetic is the same statements
// in both instantiations, so out_ctc is the same bits as the plain search's score wherever both keep the same prefixes,
// and under zero weights the two searches are the same search.
//
// LM state.  LM(p) depends on the prefix only, so it is carried per current prefix, in LDS, next to pb / pnb:
//   lm            float64, the terms of p's words added left to right;
//   ent[j-1], bo[j-1], j = 1 .. order-1:  the entry number of the LAST j words of <s> p as an n-gram (-1: not listed, or
//                 fewer than j words exist) and that n-gram's back-off.
// The term of a word w after p then needs at most `order` INDEPENDENT probes: the unigram of w (an array read) and, for
// every listed context j, the key (ent[j-1] << 32 | w) of the (j+1)-gram.  With K the length of the longest hit,
//   term = bo[order-2] + ( .. + (bo[K-1] + logp_K))        over the LISTED contexts j = K .. order-1, shortest first,
// which is the ARPA recursion unrolled; the hits are the next state.  This is exact under the one closure property the
// reader guarantees (a listed n-gram's first k-1 words are listed: an unlisted context cannot start a listed n-gram).
// Nothing is assumed about suffixes: a 3-gram may hit where the 2-gram of its last two words does not.
//
// What the fusion runs in parallel: the probes of all beam x beam extension candidates that are NEW prefixes (lane =
// pair).  A "stay" entry and an extension that lands on a prefix already in the beam keep that prefix's lm and state and
// probe nothing.  Candidates carry only the lm VALUE in registers; after the selection the <= beam winners that are new
// prefixes redo their probes (one lane each) to write the state of the next frame.
// Bound: latency.  The fusion adds two rounds of <= order-1 independent 16-byte gathers per frame into a table that does
// not fit LDS.
//
// The biasing (CTX = true) is one more prefix-only summand, total(p) + bias(p), bias(p) = hits(p) + c * k(p), read off an
// Aho-Corasick automaton over the hotword phrases (openeat_amd/utils/context_graph.py builds it).  Per current prefix, in
// LDS: the automaton state (int), hits (float64) and k = pend[state] (int).  A new-prefix candidate makes its transition in
// its own lane, next to the LM probes: the trie edge (state, token) in the edge table (ng_find), on a miss fail[state] and
// again (<= 33 dependent probes; ONE for a prefix that sits in the root), then the phrases that end in the new state, a
// chain of <= 32 (score, link) reads that is empty for most states.  State, hits and k travel in registers, so the winners
// need no second pass.  A "stay" entry and an extension that lands on a prefix already in the beam keep that prefix's
// three values and probe nothing.  Everything it adds sits under `if constexpr (CTX)`; with LM = false it also brings the
// end-of-utterance re-sort by total, which the plain search has no use for.
#include <math.h>
#include "oe_common.h"
#include "../../include/openeat_hip.h"
#include "ngram_common.h"
#include "context_common.h"

#define PB_MAXBEAM 16
#define PB_MAXC ((PB_MAXBEAM * PB_MAXBEAM + 63) / 64)          // (token, hypothesis) pairs per lane
#define PB_HASH_MUL 0x9E3779B97F4A7C15ull
#define PB_H (NG_MAXORDER - 1)                                 // LM contexts kept per prefix

__device__ __forceinline__ double pb_neg() { return -__builtin_huge_val(); }
// log_add (common.py:198-206): max + log(sum of exp(. - max)) in argument order.  exp(0) = 1 and exp(-inf) = 0 exactly, so the
// term of the maximum and the terms that are -inf are written down instead of computed: the same sum bit for bit, with one
// double-precision exp left in the common case instead of two or three (they were most of a frame's 15 us).
__device__ __forceinline__ double pb_term(double x, double m) {
    return x == m ? 1.0 : (x == pb_neg() ? 0.0 : exp(x - m));
}
__device__ __forceinline__ double pb_log_add2(double a, double b) {
    const double ninf = pb_neg();
    if (a == ninf && b == ninf) return ninf;
    const double m = fmax(a, b);
    return m + log(pb_term(a, m) + pb_term(b, m));
}
__device__ __forceinline__ double pb_log_add3(double a, double b, double c) {
    const double ninf = pb_neg();
    if (a == ninf && b == ninf && c == ninf) return ninf;
    const double m = fmax(a, fmax(b, c));
    return m + log(pb_term(a, m) + pb_term(b, m) + pb_term(c, m));
}
// (ctc + lm_weight * lm) + length_bonus * len with every product and sum rounded on its own, as a host float64 expression
// is: a fused multiply-add would move a total by an ulp and with it the order of two entries that tie exactly.
__device__ __forceinline__ double pb_total(double ctc, double lm, int len, double lm_weight, double length_bonus) {
#pragma clang fp contract(off)
    const double a = lm_weight * lm;
    const double c = length_bonus * (double)len;
    return (ctc + a) + c;
}

// total(p) of the biased search: pb_total's sum (without an LM term for LM = false), then + bias, each rounded on its own
template <bool LM>
__device__ __forceinline__ double pb_total_ctx(double ctc, double lm, int len, double lm_weight, double length_bonus, double bias) {
#pragma clang fp contract(off)
    if constexpr (LM) return pb_total(ctc, lm, len, lm_weight, length_bonus) + bias;
    const double c = length_bonus * (double)len;
    return (ctc + c) + bias;
}

// log10 p(w | the prefix whose state is ent / bo); ent_out / bo_out (or null): the state of prefix + w
__device__ __forceinline__ double pb_extend(const NgModel& m, const int* ent, const float* bo, int w, int* ent_out, float* bo_out) {
    const int H = m.order - 1;
    const float2 u = m.unigrams[w];
    int ce[PB_H], he[PB_H];
    float cb[PB_H], hl[PB_H], hb[PB_H];
#pragma unroll
    for (int j = 0; j < PB_H; ++j) {
        ce[j] = j < H ? ent[j] : -1;
        cb[j] = j < H ? bo[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < PB_H; ++j) {                               // the (j+2)-gram: context of j+1 words, then w
        he[j] = -1; hl[j] = 0.f; hb[j] = 0.f;
        if (ce[j] >= 0) {
            const unsigned long long key = ((unsigned long long)(unsigned)ce[j] << 32) | (unsigned)w;
            const long slot = ng_find(m.table, m.mask, m.max_probe, key, hl[j], hb[j]);
            if (slot >= 0) he[j] = m.n_words + (int)slot;
        }
    }
    int K = 1;
    float lp = u.x;
#pragma unroll
    for (int j = 0; j < PB_H; ++j)
        if (he[j] >= 0) { K = j + 2; lp = hl[j]; }
    double term = (double)lp;
#pragma unroll
    for (int j = 0; j < PB_H; ++j)
        if (j + 1 >= K && ce[j] >= 0) term = (double)cb[j] + term;
    if (ent_out) {
        ent_out[0] = w; bo_out[0] = u.y;
#pragma unroll
        for (int j = 1; j < PB_H; ++j) { ent_out[j] = he[j - 1]; bo_out[j] = hb[j - 1]; }
    }
    return term;
}

struct PbHyp {          // one entry of next_hyps; score: the pruning key; lm: LM only; hits, cstate, cpend: CTX only
    unsigned long long key;
    double pb, pnb, lm, score, hits;
    int len, last, parent, tok, order, cstate, cpend;
};

struct PbLmArgs {       // what the fusion takes on top of the plain search (all zero for LM = false)
    NgModel m;
    double lm_weight, length_bonus;
    int eos;
    double* __restrict__ out_ctc;
    double* __restrict__ out_lm;
};

// what the biased search takes on top of that: the context graph (openeat_hip.h; CtxGraph and the automaton's step
// pb_ctx_step: context_common.h)
struct PbCtxArgs : PbLmArgs, CtxGraph {
    int final;
    double* __restrict__ out_bias;
};
template <bool CTX> struct PbArgsOf { typedef PbLmArgs type; };          // the two searches without a graph keep their arguments
template <> struct PbArgsOf<true> { typedef PbCtxArgs type; };

// ---- the resumable search (CHUNK = true; oe_ctc_prefix_beam_chunk, semantics in include/openeat_hip.h) -------------------
// The state of a search between two chunks, device memory: a header of 8 ints (magic, B, beam, max_len, variant = LM | CTX << 1)
// and per utterance, struct of arrays over the beam slots, what the frame loop keeps in LDS - key, pb, pnb, lm, hits (8 bytes
// each), len, last, cstate, cpend, ent[PB_H], bo[PB_H] (4 bytes each) - then ncur and the frames consumed, then every slot's
// tokens and emission frames, (beam, max_len) each, INDEXED BY THE POSITION IN THE PREFIX: a slot's tail is the positions
// stable_len .. len-1 of its row, what lies in front of them is not kept up.  So committing tokens to the stable prefix moves
// nothing, and a chunk copies, per slot, the tail of the slot it grew from out of state_in and appends its own tokens.
// The size does not depend on the variant: one pair of states serves any search of that beam and max_len.
#define PB_STATE_MAGIC 0x70624353
#define PB_STATE_HEADER 32

struct PbChunkArgs {    // what the resumable search takes on top (empty for CHUNK = false)
    const void* state_in;
    void* state_out;
    int last, emit;
    int* __restrict__ stable_prefix;
    int* __restrict__ stable_frame;
    int* __restrict__ stable_len;
    int* __restrict__ out_frame;
};
struct PbNoChunk {};
template <bool CHUNK> struct PbChunkOf { typedef PbNoChunk type; };
template <> struct PbChunkOf<true> { typedef PbChunkArgs type; };

struct PbState {        // one utterance's part of a state
    unsigned long long* key;
    double *pb, *pnb, *lm, *hits;
    int *len, *last, *cstate, *cpend, *ent;
    float* bo;
    int *misc, *tail_tok, *tail_frame;
};
__host__ __device__ inline size_t pb_state_utt_bytes(int beam, int max_len) {
    return (size_t)beam * 40 + ((size_t)beam * (4 + 2 * PB_H) + 2) * 4 + (size_t)beam * (size_t)max_len * 8;
}
__device__ __forceinline__ PbState pb_state_of(const void* base, int b, int beam, int max_len) {
    char* p = (char*)base + PB_STATE_HEADER + (size_t)b * pb_state_utt_bytes(beam, max_len);
    PbState s;
    s.key = (unsigned long long*)p;
    s.pb = (double*)p + beam; s.pnb = s.pb + beam; s.lm = s.pnb + beam; s.hits = s.lm + beam;
    int* q = (int*)(s.hits + beam);
    s.len = q; s.last = q + beam; s.cstate = q + 2 * beam; s.cpend = q + 3 * beam; s.ent = q + 4 * beam;
    s.bo = (float*)(s.ent + beam * PB_H);
    s.misc = s.ent + 2 * beam * PB_H;
    s.tail_tok = s.misc + 2;
    s.tail_frame = s.tail_tok + (size_t)beam * (size_t)max_len;
    return s;
}

template <bool LM, bool CTX, bool CHUNK>
__global__ __launch_bounds__(64) void ctc_prefix_beam_kernel(const float* __restrict__ topk_logp, const long long* __restrict__ topk_idx,
                                                             int Tmax, const int* __restrict__ lens, int beam, int max_len,
                                                             typename PbArgsOf<CTX>::type la, typename PbChunkOf<CHUNK>::type ck,
                                                             int* __restrict__ hist, int* __restrict__ out_prefix,
                                                             int* __restrict__ out_len, double* __restrict__ out_score,
                                                             int* __restrict__ status) {
    __shared__ unsigned long long cur_key[PB_MAXBEAM];
    __shared__ double cur_pb[PB_MAXBEAM], cur_pnb[PB_MAXBEAM];
    __shared__ int cur_len[PB_MAXBEAM], cur_last[PB_MAXBEAM];
    __shared__ double tk_ps[PB_MAXBEAM];
    __shared__ int tk_s[PB_MAXBEAM];
    __shared__ int con_has[PB_MAXBEAM], con_from[PB_MAXBEAM], con_three[PB_MAXBEAM], con_order[PB_MAXBEAM];
    __shared__ double con_a[PB_MAXBEAM], con_b[PB_MAXBEAM];
    __shared__ unsigned long long nx_key[PB_MAXBEAM];
    __shared__ double nx_pb[PB_MAXBEAM], nx_pnb[PB_MAXBEAM];
    __shared__ int nx_len[PB_MAXBEAM], nx_last[PB_MAXBEAM];
    // LM only (never referenced, so not allocated, for LM = false)
    __shared__ double cur_lm[PB_MAXBEAM], nx_lm[PB_MAXBEAM], fin_total[PB_MAXBEAM];
    __shared__ int cur_ent[PB_MAXBEAM][PB_H], nx_ent[PB_MAXBEAM][PB_H];
    __shared__ float cur_bo[PB_MAXBEAM][PB_H], nx_bo[PB_MAXBEAM][PB_H];
    __shared__ int tk_w[PB_MAXBEAM], nx_parent[PB_MAXBEAM], nx_tok[PB_MAXBEAM];
    // CTX only (fin_total: LM or CTX)
    __shared__ double cur_hits[PB_MAXBEAM], nx_hits[PB_MAXBEAM];
    __shared__ int cur_cstate[PB_MAXBEAM], cur_cpend[PB_MAXBEAM], nx_cstate[PB_MAXBEAM], nx_cpend[PB_MAXBEAM];

    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = min(lens ? lens[b] : Tmax, Tmax);
    const double NEG = pb_neg();
    int ncur = 1;
    int t0 = 0;                                                    // CHUNK: frames consumed by the chunks before this one
    bool fresh = true;
    if constexpr (CHUNK) {
        if (ck.state_in) {                                         // resume: the header must be this call's, then LDS is reloaded
            fresh = false;
            const int* hd = (const int*)ck.state_in;
            if (hd[0] != PB_STATE_MAGIC || hd[1] != (int)gridDim.x || hd[2] != beam || hd[3] != max_len ||
                hd[4] != ((LM ? 1 : 0) | (CTX ? 2 : 0))) {
                if (lane == 0) atomicExch(status, 2);
                return;                                            // block-uniform, before any output
            }
            const PbState si = pb_state_of(ck.state_in, b, beam, max_len);
            ncur = min(max(si.misc[0], 0), beam);
            t0 = si.misc[1];
            if (lane < ncur) {
                cur_key[lane] = si.key[lane]; cur_pb[lane] = si.pb[lane]; cur_pnb[lane] = si.pnb[lane]; cur_len[lane] = si.len[lane];
                cur_last[lane] = si.last[lane];
                if constexpr (LM) {
                    cur_lm[lane] = si.lm[lane];
#pragma unroll
                    for (int j = 0; j < PB_H; ++j) { cur_ent[lane][j] = si.ent[lane * PB_H + j]; cur_bo[lane][j] = si.bo[lane * PB_H + j]; }
                }
                if constexpr (CTX) {
                    const int cs = si.cstate[lane];                // indexes the graph's tables: a state of another graph stays inside
                    cur_hits[lane] = si.hits[lane]; cur_cstate[lane] = (unsigned)cs < (unsigned)la.n_states ? cs : 0; cur_cpend[lane] = si.cpend[lane];
                }
            }
        }
    }
    if (fresh && lane == 0) {
        cur_key[0] = 0; cur_pb[0] = 0.0; cur_pnb[0] = NEG; cur_len[0] = 0; cur_last[0] = -1;
        if constexpr (LM) {
            cur_lm[0] = 0.0;
            cur_ent[0][0] = la.m.bos_word; cur_bo[0][0] = la.m.unigrams[la.m.bos_word].y;          // the context <s>
#pragma unroll
            for (int j = 1; j < PB_H; ++j) { cur_ent[0][j] = -1; cur_bo[0][j] = 0.f; }
        }
        if constexpr (CTX) { cur_hits[0] = 0.0; cur_cstate[0] = 0; cur_cpend[0] = 0; }            // the empty prefix: the root, k = 0
    }
    __syncthreads();
    int* hist_b = hist + (long)b * Tmax * beam * 2;

    for (int t = 0; t < T; ++t) {
        if (lane < beam) {
            const long o = ((long)b * Tmax + t) * beam + lane;
            const int s = (int)topk_idx[o];
            tk_ps[lane] = (double)topk_logp[o];
            tk_s[lane] = s;
            if constexpr (LM) tk_w[lane] = ng_word(la.m, s);
        }
        if (lane < ncur) con_has[lane] = 0;
        __syncthreads();

        // ---- extension candidates: pair p = (j, h), lanes p, p + 64, ...
        PbHyp cand[PB_MAXC + 1];
        bool alive[PB_MAXC + 1];
        const int npairs = beam * ncur;
#pragma unroll
        for (int c = 0; c < PB_MAXC; ++c) {
            const int p = lane + 64 * c;
            alive[c] = false;
            if (p < npairs) {
                const int j = p / ncur, h = p - j * ncur;
                const int s = tk_s[j];
                if (s != 0) {
                    const double ps = tk_ps[j];
                    const unsigned long long key = cur_key[h] * PB_HASH_MUL + (unsigned long long)(s + 1);
                    const int len = cur_len[h] + 1;
                    const bool rep = (s == cur_last[h]);
                    const double a = cur_pb[h] + ps, bb = cur_pnb[h] + ps;
                    int hit = -1;
                    for (int n = 0; n < ncur; ++n)
                        if (cur_key[n] == key && cur_len[n] == len) hit = n;
                    if (hit >= 0) {                    // lands on a prefix that is already in the beam: that prefix's lane applies it
                        con_has[hit] = 1; con_from[hit] = h; con_three[hit] = rep ? 0 : 1; con_a[hit] = a; con_b[hit] = bb;
                        con_order[hit] = 2 * p + 1;
                    } else {
                        alive[c] = true;
                        cand[c].key = key; cand[c].len = len; cand[c].last = s; cand[c].parent = h; cand[c].tok = s;
                        cand[c].pb = NEG;
                        cand[c].pnb = rep ? a : pb_log_add3(NEG, a, bb);
                        cand[c].order = 2 * p + 1;
                        if constexpr (LM) cand[c].lm = cur_lm[h] + pb_extend(la.m, cur_ent[h], cur_bo[h], tk_w[j], nullptr, nullptr);
                        if constexpr (CTX) {
                            double hits = cur_hits[h];
                            const int ns = pb_ctx_step(la, cur_cstate[h], s, hits);
                            cand[c].hits = hits; cand[c].cstate = ns; cand[c].cpend = la.pend[ns];
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- the current prefixes' own entries: lane n
        alive[PB_MAXC] = false;
        if (lane < ncur) {
            const int n = lane;
            const double pb = cur_pb[n], pnb = cur_pnb[n];
            const int last = cur_last[n];
            int j0 = -1, jr = -1;
            for (int j = 0; j < beam; ++j) {
                if (tk_s[j] == 0 && j0 < 0) j0 = j;
                if (tk_s[j] == last && last > 0 && jr < 0) jr = j;
            }
            double npb = NEG, npnb = NEG;
            int order = 0x7fffffff;
            bool touched = false;
            if (j0 >= 0) {
                npb = pb_log_add3(NEG, pb + tk_ps[j0], pnb + tk_ps[j0]);
                order = min(order, 2 * (j0 * ncur + n));
                touched = true;
            }
            const bool rep = jr >= 0, con = con_has[n] != 0;
            const bool con_first = con && (!rep || con_from[n] < n);
            if (con && con_first) npnb = con_three[n] ? pb_log_add3(npnb, con_a[n], con_b[n]) : pb_log_add2(npnb, con_a[n]);
            if (rep) { npnb = pb_log_add2(npnb, pnb + tk_ps[jr]); order = min(order, 2 * (jr * ncur + n)); touched = true; }
            if (con && !con_first) npnb = con_three[n] ? pb_log_add3(npnb, con_a[n], con_b[n]) : pb_log_add2(npnb, con_a[n]);
            if (con) { order = min(order, con_order[n]); touched = true; }
            if (touched) {
                alive[PB_MAXC] = true;
                PbHyp& e = cand[PB_MAXC];
                e.key = cur_key[n]; e.len = cur_len[n]; e.last = last; e.parent = n; e.tok = -1; e.pb = npb; e.pnb = npnb; e.order = order;
                if constexpr (LM) e.lm = cur_lm[n];
                if constexpr (CTX) { e.hits = cur_hits[n]; e.cstate = cur_cstate[n]; e.cpend = cur_cpend[n]; }
            }
        }
#pragma unroll
        for (int c = 0; c <= PB_MAXC; ++c)
            if (alive[c]) {
                cand[c].score = pb_log_add2(cand[c].pb, cand[c].pnb);
                if constexpr (CTX)
                    cand[c].score = pb_total_ctx<LM>(cand[c].score, cand[c].lm, cand[c].len, la.lm_weight, la.length_bonus,
                                                     pb_bias(cand[c].hits, la.c, cand[c].cpend));
                else if constexpr (LM) cand[c].score = pb_total(cand[c].score, cand[c].lm, cand[c].len, la.lm_weight, la.length_bonus);
            }

        // ---- the best `beam` entries by (score descending, first touch ascending)
        int nsel = 0;
        for (int r = 0; r < beam; ++r) {
            double bs = NEG;
            int bo = 0x7fffffff, bc = -1;
#pragma unroll
            for (int c = 0; c <= PB_MAXC; ++c)
                if (alive[c] && (bc < 0 || cand[c].score > bs || (cand[c].score == bs && cand[c].order < bo))) { bs = cand[c].score; bo = cand[c].order; bc = c; }
            double ws = bs;
            int wo = bo;                                      // lanes without a candidate carry (NEG, INT_MAX)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double os = oe_shfl_xor_f64(ws, o);
                const int oo = __shfl_xor(wo, o, 64);
                if (oo != 0x7fffffff && (wo == 0x7fffffff || os > ws || (os == ws && oo < wo))) { ws = os; wo = oo; }
            }
            if (wo == 0x7fffffff) break;                      // nothing left (wave-uniform)
            if (bc >= 0 && bo == wo) {                        // stamps are unique: this lane holds the winner
#pragma unroll
                for (int c = 0; c <= PB_MAXC; ++c)
                    if (c == bc) {
                        nx_key[r] = cand[c].key; nx_pb[r] = cand[c].pb; nx_pnb[r] = cand[c].pnb; nx_len[r] = cand[c].len; nx_last[r] = cand[c].last;
                        if constexpr (LM) { nx_lm[r] = cand[c].lm; nx_parent[r] = cand[c].parent; nx_tok[r] = cand[c].tok; }
                        if constexpr (CTX) { nx_hits[r] = cand[c].hits; nx_cstate[r] = cand[c].cstate; nx_cpend[r] = cand[c].cpend; }
                        hist_b[((long)t * beam + r) * 2] = cand[c].parent;
                        hist_b[((long)t * beam + r) * 2 + 1] = cand[c].tok;
                        alive[c] = false;
                    }
            }
            nsel = r + 1;
        }
        __syncthreads();
        if constexpr (LM) {
            // ---- the winners' LM state: a new prefix redoes its probes, any other entry keeps its prefix's state
            if (lane < nsel) {
                const int par = nx_parent[lane], tok = nx_tok[lane];
                if (tok >= 0) {
                    pb_extend(la.m, cur_ent[par], cur_bo[par], ng_word(la.m, tok), nx_ent[lane], nx_bo[lane]);
                } else {
#pragma unroll
                    for (int j = 0; j < PB_H; ++j) { nx_ent[lane][j] = cur_ent[par][j]; nx_bo[lane][j] = cur_bo[par][j]; }
                }
            }
            __syncthreads();
        }
        if (lane < nsel) {
            cur_key[lane] = nx_key[lane]; cur_pb[lane] = nx_pb[lane]; cur_pnb[lane] = nx_pnb[lane]; cur_len[lane] = nx_len[lane];
            cur_last[lane] = nx_last[lane];
            if constexpr (LM) {
                cur_lm[lane] = nx_lm[lane];
#pragma unroll
                for (int j = 0; j < PB_H; ++j) { cur_ent[lane][j] = nx_ent[lane][j]; cur_bo[lane][j] = nx_bo[lane][j]; }
            }
            if constexpr (CTX) { cur_hits[lane] = nx_hits[lane]; cur_cstate[lane] = nx_cstate[lane]; cur_cpend[lane] = nx_cpend[lane]; }
        }
        ncur = nsel;
        __syncthreads();
    }

    // ---- LM / CTX, end of the utterance: the </s> term, the pending credit dropped if final, then the survivors stably
    // re-sorted by total
    // CHUNK, not the last chunk: neither of the two, so the totals are the running ones the pruning key saw and the order stays
    bool ended = true;
    if constexpr (CHUNK) ended = ck.last != 0;
    double lm = 0.0, ctc = NEG, total = NEG, bias = 0.0;
    if constexpr (LM || CTX) {
        if (lane < ncur) {
            if constexpr (LM) {
                lm = cur_lm[lane];
                if (la.eos && ended) lm = lm + pb_extend(la.m, cur_ent[lane], cur_bo[lane], la.m.eos_word, nullptr, nullptr);
            }
            ctc = pb_log_add2(cur_pb[lane], cur_pnb[lane]);
            if constexpr (CTX) {
                bias = (la.final && ended) ? cur_hits[lane] : pb_bias(cur_hits[lane], la.c, cur_cpend[lane]);
                total = pb_total_ctx<LM>(ctc, lm, cur_len[lane], la.lm_weight, la.length_bonus, bias);
            } else {
                total = pb_total(ctc, lm, cur_len[lane], la.lm_weight, la.length_bonus);
            }
            fin_total[lane] = total;
        }
        __syncthreads();
    }

    if constexpr (CHUNK) {
        // ---- the end of a chunk.  Every slot's row of tokens and frames (position-indexed) is put together where it will
        // stay: in state_out, or, without one (the last chunk only), directly in its rank's rows of out_prefix / out_frame.
        __shared__ int fin_org[PB_MAXBEAM], fin_row[PB_MAXBEAM];
        const bool outw = ck.last || ck.emit;
        const bool keep = ck.state_out != nullptr;
        const int S0 = fresh ? 0 : min(max(ck.stable_len[b], 0), max_len);          // committed so far
        const long ub = (long)b * beam;
        PbState si{}, so{};
        if (!fresh) si = pb_state_of(ck.state_in, b, beam, max_len);
        if (keep) so = pb_state_of(ck.state_out, b, beam, max_len);
        // (A) lane = slot: the scores, then the chunk's back-pointers walked to its first frame: the tokens it appended go to
        // their positions, and the slot of state_in the prefix grew from is what is left
        if (lane < beam) {
            if (lane < ncur) {
                int rank = lane;
                if constexpr (LM || CTX) {
                    rank = 0;
                    for (int i = 0; i < ncur; ++i) {
                        const double ti = fin_total[i];
                        if (ti > total || (ti == total && i < lane)) ++rank;
                    }
                }
                const long o = ub + rank;
                const int len = cur_len[lane];
                if (outw) {
                    if constexpr (CTX) {
                        out_score[o] = total;
                        la.out_ctc[o] = ctc;
                        if constexpr (LM) la.out_lm[o] = lm;
                        la.out_bias[o] = bias;
                    } else if constexpr (LM) {
                        out_score[o] = total;
                        la.out_ctc[o] = ctc;
                        la.out_lm[o] = lm;
                    } else {
                        out_score[o] = pb_log_add2(cur_pb[lane], cur_pnb[lane]);
                    }
                    out_len[o] = len;
                }
                if (len > max_len) atomicExch(status, 1);
                int* dtok = keep ? so.tail_tok + (size_t)lane * max_len : out_prefix + o * max_len;
                int* dfr = keep ? so.tail_frame + (size_t)lane * max_len : (ck.out_frame ? ck.out_frame + o * max_len : nullptr);
                int slot = lane, pos = len - 1;
                for (int t = T - 1; t >= 0; --t) {
                    const int parent = hist_b[((long)t * beam + slot) * 2], tok = hist_b[((long)t * beam + slot) * 2 + 1];
                    if (tok >= 0) {
                        if (pos >= 0 && pos < max_len) {
                            dtok[pos] = tok;
                            if (dfr) dfr[pos] = t0 + t;
                        }
                        --pos;
                    }
                    slot = parent;
                }
                fin_org[lane] = slot;
                fin_row[lane] = rank;
            } else if (outw) {
                const long o = ub + lane;
                out_score[o] = NEG;
                if constexpr (LM) { la.out_ctc[o] = NEG; la.out_lm[o] = NEG; }
                if constexpr (CTX) {
                    if constexpr (!LM) la.out_ctc[o] = NEG;
                    la.out_bias[o] = NEG;
                }
                out_len[o] = -1;
            }
        }
        __syncthreads();
        // (B) the wave, slot by slot: the tail the prefix had when the chunk began, copied from the slot it grew from
        if (!fresh) {
            for (int s = 0; s < ncur; ++s) {
                const int org = fin_org[s];
                const int ol = min(si.len[org], max_len);
                const long o = ub + fin_row[s];
                int* dtok = keep ? so.tail_tok + (size_t)s * max_len : out_prefix + o * max_len;
                int* dfr = keep ? so.tail_frame + (size_t)s * max_len : (ck.out_frame ? ck.out_frame + o * max_len : nullptr);
                const int* stok = si.tail_tok + (size_t)org * max_len;
                const int* sfr = si.tail_frame + (size_t)org * max_len;
                for (int i0 = S0 + lane; i0 < ol; i0 += 64 * 8) {   // 16 independent loads in flight: one wave moves the whole tail
                    int vt[8], vf[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + 64 * u;
                        vt[u] = i < ol ? stok[i] : 0;
                        vf[u] = i < ol ? sfr[i] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + 64 * u;
                        if (i < ol) {
                            dtok[i] = vt[u];
                            if (dfr) dfr[i] = vf[u];
                        }
                    }
                }
            }
        }
        __syncthreads();
        // (C) the stable prefix grows by what all live prefixes share behind it (lane = position, 64 at a time); where their
        // chains disagree about a token's frame, the earliest one is committed
        int S1 = S0;
        if (keep && ncur > 0) {
            int minlen = max_len;
            for (int s = 0; s < ncur; ++s) minlen = min(minlen, cur_len[s]);
            S1 = max(minlen, S0);
            for (int base = S0; base < minlen; base += 64) {
                const int i = base + lane;
                bool differ = false;
                int tok0 = 0, fmin = 0;
                if (i < minlen) {
                    tok0 = so.tail_tok[i]; fmin = so.tail_frame[i];
                    for (int s = 1; s < ncur; ++s) {
                        if (so.tail_tok[(size_t)s * max_len + i] != tok0) differ = true;
                        fmin = min(fmin, so.tail_frame[(size_t)s * max_len + i]);
                    }
                }
                const unsigned long long m = __ballot(differ);
                const int first = m ? __ffsll((long long)m) - 1 : 64;
                if (i < minlen && lane < first) {
                    ck.stable_prefix[(long)b * max_len + i] = tok0;
                    ck.stable_frame[(long)b * max_len + i] = fmin;
                }
                if (m) { S1 = base + first; break; }
            }
            if (lane == 0) ck.stable_len[b] = S1;
        }
        __syncthreads();
        // (D) the n-best rows: the stable prefix, then the slot's own row
        if (outw) {
            for (int s = 0; s < ncur; ++s) {
                if (cur_len[s] > max_len) continue;                // reported; the row is not written, as in the one-shot search
                const long o = ub + fin_row[s];
                const int n = keep ? cur_len[s] : S1;              // without a state (S1 = S0) the positions behind are in place already
                const int* rtok = so.tail_tok + (size_t)s * max_len;
                const int* rfr = so.tail_frame + (size_t)s * max_len;
                for (int i = lane; i < n; i += 64) {
                    out_prefix[o * max_len + i] = i < S1 ? ck.stable_prefix[(long)b * max_len + i] : rtok[i];
                    if (ck.out_frame) ck.out_frame[o * max_len + i] = i < S1 ? ck.stable_frame[(long)b * max_len + i] : rfr[i];
                }
            }
        }
        // (E) what the frame loop carries
        if (keep) {
            if (lane < ncur) {
                so.key[lane] = cur_key[lane]; so.pb[lane] = cur_pb[lane]; so.pnb[lane] = cur_pnb[lane]; so.len[lane] = cur_len[lane];
                so.last[lane] = cur_last[lane];
                if constexpr (LM) {
                    so.lm[lane] = cur_lm[lane];
#pragma unroll
                    for (int j = 0; j < PB_H; ++j) { so.ent[lane * PB_H + j] = cur_ent[lane][j]; so.bo[lane * PB_H + j] = cur_bo[lane][j]; }
                }
                if constexpr (CTX) { so.hits[lane] = cur_hits[lane]; so.cstate[lane] = cur_cstate[lane]; so.cpend[lane] = cur_cpend[lane]; }
            }
            if (lane == 0) {
                so.misc[0] = ncur; so.misc[1] = t0 + max(T, 0);
                if (b == 0) {
                    int* hd = (int*)ck.state_out;
                    hd[0] = PB_STATE_MAGIC; hd[1] = (int)gridDim.x; hd[2] = beam; hd[3] = max_len; hd[4] = (LM ? 1 : 0) | (CTX ? 2 : 0);
                    hd[5] = 0; hd[6] = 0; hd[7] = 0;
                }
            }
        }
        return;
    }

    // ---- results: scores, lengths, tokens by walking the back-pointers
    if (lane < beam) {
        if (lane < ncur) {
            int rank = lane;
            if constexpr (LM || CTX) {
                rank = 0;
                for (int i = 0; i < ncur; ++i) {
                    const double ti = fin_total[i];
                    if (ti > total || (ti == total && i < lane)) ++rank;
                }
            }
            const long o = (long)b * beam + rank;
            const int len = cur_len[lane];
            if constexpr (CTX) {
                out_score[o] = total;
                la.out_ctc[o] = ctc;
                if constexpr (LM) la.out_lm[o] = lm;
                la.out_bias[o] = bias;
            } else if constexpr (LM) {
                out_score[o] = total;
                la.out_ctc[o] = ctc;
                la.out_lm[o] = lm;
            } else {
                out_score[o] = pb_log_add2(cur_pb[lane], cur_pnb[lane]);
            }
            out_len[o] = len;
            if (len > max_len) { atomicExch(status, 1); return; }
            int slot = lane, pos = len - 1;
            for (int t = T - 1; t >= 0 && pos >= 0; --t) {
                const int parent = hist_b[((long)t * beam + slot) * 2], tok = hist_b[((long)t * beam + slot) * 2 + 1];
                if (tok >= 0) out_prefix[o * max_len + pos--] = tok;
                slot = parent;
            }
        } else {
            const long o = (long)b * beam + lane;
            out_score[o] = NEG;
            if constexpr (LM) { la.out_ctc[o] = NEG; la.out_lm[o] = NEG; }
            if constexpr (CTX) {
                if constexpr (!LM) la.out_ctc[o] = NEG;
                la.out_bias[o] = NEG;
            }
            out_len[o] = -1;
        }
    }
}

// back-pointer words of the workspace; one status word follows them
static size_t pb_hist_words(int B, int Tmax, int beam) { return (size_t)B * (size_t)max(Tmax, 1) * (size_t)beam * 2; }

extern "C" size_t oe_ctc_prefix_beam_workspace_bytes(int B, int Tmax, int beam) { return (pb_hist_words(B, Tmax, beam) + 1) * sizeof(int); }

// la: a PbCtxArgs; the two instantiations without a graph take its PbLmArgs part
template <bool LM, bool CTX, bool CHUNK>
static int pb_launch(const oe_prefix_beam_args& a, const typename PbArgsOf<CTX>::type& la, const typename PbChunkOf<CHUNK>::type& ck, void* stream) {
    int* hist = (int*)a.workspace;
    int* status = hist + pb_hist_words(a.B, a.Tmax, a.beam);      // the caller zeroes this word and reads it back
    hipLaunchKernelGGL((ctc_prefix_beam_kernel<LM, CTX, CHUNK>), dim3(a.B), dim3(64), 0, (hipStream_t)stream, a.topk_logp, a.topk_idx, a.Tmax,
                       a.lens, a.beam, a.max_len, la, ck, hist, a.out_prefix, a.out_len, a.out_score, status);
    OE_LAUNCH_CHECK(CHUNK ? "ctc_prefix_beam_chunk" : "ctc_prefix_beam");
    return 0;
}

// the checks of the search's arguments, shared by the two entry points; fills la
static int pb_prepare(const char* fn, const oe_prefix_beam_args& a, PbCtxArgs& la) {
    const oe_ngram_model* lm = a.lm;
    const oe_context_graph* g = a.ctx;
    OE_REQUIRE(a.topk_logp && a.topk_idx && a.workspace && a.out_prefix && a.out_len && a.out_score, "%s: null pointer", fn);
    OE_REQUIRE((!lm && !g) || a.out_ctc, "%s: null pointer (out_ctc)", fn);
    OE_REQUIRE(!lm || a.out_lm, "%s: null pointer (out_lm)", fn);
    OE_REQUIRE(!g || a.out_bias, "%s: null pointer (out_bias)", fn);
    OE_REQUIRE(!lm || (lm->unigrams && lm->table && lm->tok2word), "%s: null pointer (model)", fn);
    OE_REQUIRE(!g || (g->edges && g->fail && g->out && g->pend), "%s: null pointer (context graph)", fn);
    OE_REQUIRE(a.B > 0 && a.Tmax >= 0 && a.max_len >= 0, "%s: bad shape B=%d Tmax=%d max_len=%d", fn, a.B, a.Tmax, a.max_len);
    OE_REQUIRE(a.beam >= 1 && a.beam <= PB_MAXBEAM, "%s: beam must be 1..%d (got %d)", fn, PB_MAXBEAM, a.beam);
    if (lm) {
        if (ng_model_args(fn, lm, &la.m)) return -1;
        OE_REQUIRE(lm->V > 0, "%s: bad vocabulary size V=%d", fn, lm->V);
        OE_REQUIRE(isfinite(a.lm_weight), "%s: lm_weight must be finite", fn);
        la.lm_weight = a.lm_weight; la.eos = a.eos; la.out_lm = a.out_lm;
    }
    if (lm || g) {
        OE_REQUIRE(isfinite(a.length_bonus), "%s: length_bonus must be finite", fn);
        la.length_bonus = a.length_bonus; la.out_ctc = a.out_ctc;
    } else {
        OE_REQUIRE(a.lm_weight == 0.0 && a.length_bonus == 0.0,
                   "%s: the plain search has no lm_weight or length_bonus term (got %g and %g): both must be 0", fn, a.lm_weight, a.length_bonus);
    }
    if (g) {
        if (ctx_graph_args(fn, g, &la)) return -1;
        la.final = a.final; la.out_bias = a.out_bias;
    }
    return 0;
}

extern "C" int oe_ctc_prefix_beam(const oe_prefix_beam_args* args, void* stream) {
    const char* fn = "oe_ctc_prefix_beam";
    OE_REQUIRE(args, "%s: null pointer (args)", fn);
    const oe_prefix_beam_args& a = *args;
    PbCtxArgs la{};
    if (pb_prepare(fn, a, la)) return -1;
    const PbNoChunk ck{};
    if (!a.lm && !a.ctx) return pb_launch<false, false, false>(a, la, ck, stream);
    if (!a.ctx) return pb_launch<true, false, false>(a, la, ck, stream);
    return a.lm ? pb_launch<true, true, false>(a, la, ck, stream) : pb_launch<false, true, false>(a, la, ck, stream);
}

extern "C" size_t oe_ctc_prefix_beam_state_bytes(int B, int beam, int max_len) {
    if (B <= 0 || beam < 1 || beam > PB_MAXBEAM || max_len < 0) return 0;
    return PB_STATE_HEADER + (size_t)B * pb_state_utt_bytes(beam, max_len);
}

extern "C" int oe_ctc_prefix_beam_chunk(const oe_prefix_beam_chunk* chunk, void* stream) {
    const char* fn = "oe_ctc_prefix_beam_chunk";
    OE_REQUIRE(chunk, "%s: null pointer (chunk)", fn);
    OE_REQUIRE(chunk->search, "%s: null pointer (search)", fn);
    const oe_prefix_beam_args& a = *chunk->search;
    PbCtxArgs la{};
    if (pb_prepare(fn, a, la)) return -1;
    OE_REQUIRE(chunk->state_out || chunk->last, "%s: state_out may be NULL with last only", fn);
    OE_REQUIRE(!chunk->state_in || chunk->state_in != chunk->state_out, "%s: state_in and state_out must not alias", fn);
    OE_REQUIRE(chunk->stable_prefix && chunk->stable_frame && chunk->stable_len, "%s: null pointer (stable_prefix / stable_frame / stable_len)", fn);
    PbChunkArgs ck{};
    ck.state_in = chunk->state_in; ck.state_out = chunk->state_out; ck.last = chunk->last != 0; ck.emit = chunk->emit != 0;
    ck.stable_prefix = chunk->stable_prefix; ck.stable_frame = chunk->stable_frame; ck.stable_len = chunk->stable_len;
    ck.out_frame = chunk->out_frame;
    if (!a.lm && !a.ctx) return pb_launch<false, false, true>(a, la, ck, stream);
    if (!a.ctx) return pb_launch<true, false, true>(a, la, ck, stream);
    return a.lm ? pb_launch<true, true, true>(a, la, ck, stream) : pb_launch<false, true, true>(a, la, ck, stream);
}
